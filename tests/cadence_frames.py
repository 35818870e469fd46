"""Container streams for the cadence API's tests: a moving clip with a cut in it (the textures of fldr_harness.synthetic_pair, as in
tests/test_gpu_pipe.py), expanded by a pulldown pattern, every repeated instance perturbed by +-1 code of y8 on at most 8 luma samples —
what a re-encode leaves of a repeat.  Shared by tests/test_cadence_cpu.py, which asserts on the CPU that the perturbation leaves the
oracle's survivors equal to the first instance of every run, and tests/test_gpu_cadence.py, which relies on it."""
import functools

import numpy as np

import cadence_oracle as C
import rate_frames as RF

H, W = 256, 448                                   # the size of tests/test_gpu_pipe.py
N_REAL, CUT_AT = 12, 3                            # real frames; the first frame of the second scene
# pattern -> (cycle, drop, times each real frame is shown, repeating)
PATTERNS = {"3:2": (5, 3, (3, 2)), "2:2": (2, 1, (2,)), "4+1": (5, 1, (1, 1, 1, 2))}
FORMATS = [("nv12", 8), ("i420", 10)]             # NV12 and yuv420p10le


def _clip(n, seed):
    """n frames of a texture moving 4 px down and 6 px right per frame (BGR planar numpy)."""
    import fldr_harness as Hn
    base = Hn.synthetic_pair(H + 4 * n, W + 6 * n, seed=seed).numpy()[0]
    return [np.ascontiguousarray(base[:, 4 * k:4 * k + H, 6 * k:6 * k + W]) for k in range(n)]


@functools.lru_cache(maxsize=None)
def real_frames(layout, depth):
    """N_REAL frames in the container: CUT_AT of one moving texture, then another, darker one."""
    a, b = _clip(CUT_AT, seed=5), _clip(N_REAL - CUT_AT, seed=11)
    bgr = a + [(f.astype(np.float64) * 0.35).round().astype(np.uint8) for f in b]
    return [RF.planes_of_bgr(f, layout, depth) for f in bgr]


def perturbed(planes, layout, depth, seed):
    """A copy of a frame with 1 .. 8 luma samples moved by one code of y8 (up where the sample is dark, down where it is bright)."""
    g = np.random.default_rng(seed)
    y = planes[0].copy()
    step = 1 if depth == 8 else (1 << 8 if layout == "nv12" else 1 << 2)
    for _ in range(int(g.integers(1, 9))):
        r, c = int(g.integers(0, y.shape[0])), int(g.integers(0, y.shape[1]))
        dark = C.S.y8(y[r:r + 1, c:c + 1], layout, depth)[0, 0] < 128
        y[r, c] = y[r, c] + step if dark else y[r, c] - step
    return (y,) + tuple(planes[1:])


@functools.lru_cache(maxsize=None)
def stream(pattern, layout, depth, n_container, first_real=0, first_instance=0):
    """-> (frames, source): n_container frames, source[n] = (real frame number, instance).  first_real / first_instance: where in the
    pattern the stream starts (first_instance > 0: inside a run of repeats).  Frames are shared: never written."""
    counts = PATTERNS[pattern][2]
    real = real_frames(layout, depth)
    frames, source = [], []
    k, inst = first_real, first_instance
    while len(frames) < n_container:
        f = real[k] if inst == 0 else perturbed(real[k], layout, depth, seed=1000 * k + inst)
        for p in f:
            p.flags.writeable = False
        frames.append(f)
        source.append((k, inst))
        inst += 1
        if inst == counts[k % len(counts)]:
            k, inst = k + 1, 0
    return frames, source


def measures(frames, layout, depth, tile_sad_min=0):
    """The oracle's result of every pair (n - 1, n); [0] is None."""
    return [None] + [C.measure(frames[n - 1], frames[n], (layout, depth), tile_sad_min) for n in range(1, len(frames))]
