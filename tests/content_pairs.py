"""Seeded frame pairs with the content of real video that fldr_harness.synthetic_pair's texture never has: black, flat and fading
frames, scene cuts, letterbox bars, clipped highlights and shadows, sensor grain, pans far beyond the other tests' motions, fine
periodic detail and a small object on a flat background.

Every generator returns a uint8 [2,3,H,W] pair (I0, I1; B, G, R planes, as synthetic_pair) that depends only on (H, W, seed).  The
texture is fldr_harness.texture (synthetic_pair's 1/f texture, 0..1).  "Moving (dx, dy) px" means what it means in synthetic_pair:
I1[y, x] = I0[y + dy, x + dx] wherever both sides lie in the frame."""
import numpy as np
import torch

import fldr_harness as Hn

LETTERBOX_ASPECT = 2.39
LETTERBOX_LEVEL = 16                   # limited-range black
FLAT_BGR = (90, 128, 200)
OBJECT_BG_BGR = (60, 100, 140)
OBJECT_SIZE, OBJECT_SHIFT = 64, 40
SHIFT = (6, 4)                         # (dx, dy): synthetic_pair's motion
GRAIN_SIGMA = 10.0                     # levels
STRIPE_PERIOD, STRIPE_ON, STRIPE_SHIFT = 5, 2, 3


def _u8(a):
    """[1,3,H,W] or [3,H,W] float in 0..1 -> uint8 [3,H,W]."""
    return (a.reshape(3, *a.shape[-2:]).clamp(0, 1) * 255).round().to(torch.uint8)


def _pair(a, b):
    return torch.stack([a, b], 0).contiguous()


def _moving(H, W, seed, dx=SHIFT[0], dy=SHIFT[1], fn=None):
    """(I0, I1) as float [3,H,W] views of one texture, I1 = I0 moved by (dx, dy); fn maps the texture first."""
    base = Hn.texture(H + dy, W + dx, seed)[0]
    if fn is not None:
        base = fn(base)
    return base[:, :H, :W], base[:, dy:dy + H, dx:dx + W]


def letterbox_rows(H, W):
    """(top, bottom): the number of bar rows above and below a 2.39:1 picture (138 / 139 at 1920x1080, 276 / 277 at 3840x2160)."""
    active = min(H, int(round(W / LETTERBOX_ASPECT)))
    top = (H - active) // 2
    return top, H - active - top


def black(H, W, seed=0):
    return torch.zeros(2, 3, H, W, dtype=torch.uint8)


def flat(H, W, seed=0):
    return torch.tensor(FLAT_BGR, dtype=torch.uint8).view(1, 3, 1, 1).expand(2, 3, H, W).contiguous()


def fade_in(H, W, seed=0):
    """From black to the texture."""
    return _pair(torch.zeros(3, H, W, dtype=torch.uint8), _u8(Hn.texture(H, W, seed)))


def fade(H, W, seed=0):
    """I1 = round(0.6 I0), no motion (0.6 x of an integer x is never a tie)."""
    I0 = _u8(Hn.texture(H, W, seed))
    return _pair(I0, (I0.double() * 0.6).round().to(torch.uint8))


def cut(H, W, seed=0):
    """Two unrelated textures."""
    return _pair(_u8(Hn.texture(H, W, seed)), _u8(Hn.texture(H, W, seed + 7919)))


def letterbox(H, W, seed=0):
    """The texture moving (6, 4) px inside 2.39:1 bars of constant 16, the same bars in both frames."""
    I0, I1 = (_u8(f) for f in _moving(H, W, seed))
    top, bottom = letterbox_rows(H, W)
    for f in (I0, I1):
        f[:, :top] = LETTERBOX_LEVEL
        f[:, H - bottom:] = LETTERBOX_LEVEL
    return _pair(I0, I1)


def clipped(H, W, seed=0):
    """The texture moving (6, 4) px, stretched so that its lower quartile maps to 0 and its upper quartile to 1, then clipped: a quarter
    of the pixels saturated at each end, bordered by steep edges.  (A fixed 3 x texture - 1 saturates only 6 .. 25 % at an end: the
    texture's quartiles move with the frame size.)"""
    def fn(b):
        lo, hi = np.quantile(b.numpy(), [0.25, 0.75])
        return ((b - float(lo)) / float(hi - lo)).clamp(0, 1)
    I0, I1 = _moving(H, W, seed, fn=fn)
    return _pair(_u8(I0), _u8(I1))


def grain(H, W, seed=0):
    """The texture moving (6, 4) px plus independent Gaussian noise of sigma 10 levels in each frame."""
    I0, I1 = _moving(H, W, seed)
    g = torch.Generator().manual_seed(seed + 104729)
    noisy = lambda f: _u8(f + torch.randn(f.shape, generator=g, dtype=torch.float64).float() * (GRAIN_SIGMA / 255.0))
    return _pair(noisy(I0), noisy(I1))


def pan_shift(H, W):
    """(dx, dy) of the pan: (W / 12, H / 12), 320 x 180 px at 3840x2160."""
    return W // 12, H // 12


def pan(H, W, seed=0):
    """A global shift of (W / 12, H / 12) px."""
    dx, dy = pan_shift(H, W)
    I0, I1 = _moving(H, W, seed, dx, dy)
    return _pair(_u8(I0), _u8(I1))


def stripes(H, W, seed=0):
    """Vertical stripes, period 5 px (2 on, 3 off) at full contrast over a low-contrast texture, moving 3 px horizontally: the match is
    ambiguous (+3 or -2 px)."""
    def fn(b):
        on = (torch.arange(b.shape[-1]) % STRIPE_PERIOD < STRIPE_ON).float()
        return on * 0.8 + b * 0.2
    I0, I1 = _moving(H, W, seed, STRIPE_SHIFT, 0, fn)
    return _pair(_u8(I0), _u8(I1))


def object_box(H, W):
    """(y0, x0): the top-left corner of the block in I0; in I1 it sits OBJECT_SHIFT px further right."""
    return H // 2 - OBJECT_SIZE // 2, W // 2 - OBJECT_SIZE // 2 - OBJECT_SHIFT // 2


def object_block(H, W, seed=0):
    """A flat background with one textured 64 x 64 block moving 40 px to the right."""
    out = torch.tensor(OBJECT_BG_BGR, dtype=torch.uint8).view(1, 3, 1, 1).expand(2, 3, H, W).contiguous()
    blk = _u8(Hn.texture(OBJECT_SIZE, OBJECT_SIZE, seed))
    y0, x0 = object_box(H, W)
    out[0, :, y0:y0 + OBJECT_SIZE, x0:x0 + OBJECT_SIZE] = blk
    out[1, :, y0:y0 + OBJECT_SIZE, x0 + OBJECT_SHIFT:x0 + OBJECT_SHIFT + OBJECT_SIZE] = blk
    return out


CASES = {"black": black, "flat": flat, "fade_in": fade_in, "fade": fade, "cut": cut, "letterbox": letterbox, "clipped": clipped,
         "grain": grain, "pan": pan, "stripes": stripes, "object": object_block}


def pair(case, H, W, seed=0):
    """uint8 [2,3,H,W] of the named case."""
    return CASES[case](H, W, seed)
