"""What the CPU tests of the C libraries (test_native_model_cpu, test_video_cpu, test_video10_cpu, test_rate_cpu) all ask of a built
library: the names a header declares, the dynamic symbols of the .so, and the disassembly of its gfx950 code objects."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared(path, macro):
    """The fldr_* functions the header at `path` declares behind the export macro `macro`."""
    return set(re.findall(macro + r"\s+[^;(]*?\b(fldr_[a-z0-9_]+)\s*\(", open(path).read()))


def syms(lib, args):
    """The dynamic symbol names of `lib` (`nm -D` + args, e.g. ["--defined-only"])."""
    out = subprocess.run(["nm", "-D"] + args + [lib], capture_output=True, text=True, check=True).stdout
    return set(l.split()[-1] for l in out.splitlines() if l.strip())


def disassemble(lib):
    """llvm-objdump -d of every code object bundled in `lib`: one text per code object."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources as KR
    out = []
    for blob in KR.code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(blob)
            f.flush()
            out.append(subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "-d", f.name], capture_output=True, text=True, check=True).stdout)
    return out
