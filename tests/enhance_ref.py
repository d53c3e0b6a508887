"""Low-light enhancement restated in numpy: tile-adaptive, contrast-limited histogram equalisation of luma applied as a hue-preserving gain
(DESIGN.md "Low-light detection").  Exact integer arithmetic throughout; rf_enhance_host and the kernels must agree to the byte.

    Y        (77 R + 150 G + 29 B + 128) >> 8 of a BGR pixel
    tiles    ceil(rows / T) x ceil(cols / T), tile (j, i) = rows [jT, min((j + 1)T, rows)), columns likewise, n pixels
    LUT      h = luma histogram, c = inclusive prefix sum, p99 = smallest v with 100 c[v] >= 99 n
             p99 >= dark_below: identity, flag 0
             else flag 1: lim = max(1, (clip n) >> 16), ex = sum max(h - lim, 0), h = min(h, lim) + ex // 256 + (v < ex % 256),
             LUT[v] = max(v, (2 * 255 * c[v] + n) // (2 n))
    pixel    per axis with D = 2T: p = 2y + 1 - T, q = floor(p / D), a0 = clamp(q), a1 = clamp(q + 1), w = 0 if p < 0 else p mod D
             v = sum of the four LUT values at Y times their weights, Yn = (2 v + D^2) // (2 D^2)
    gain     Yn == Y: copied; else c -> min(255, (2 c Yn + Yd) // (2 Yd)), Yd = max(Y, 1)
"""
import numpy as np

DEFAULTS = dict(tile=64, clip=2048, dark_below=64)


def resolve(tile=0, clip=0, dark_below=0):
    return tile or DEFAULTS["tile"], clip or DEFAULTS["clip"], dark_below or DEFAULTS["dark_below"]


def luma(frame: np.ndarray) -> np.ndarray:
    f = frame.astype(np.int64)
    return (77 * f[..., 2] + 150 * f[..., 1] + 29 * f[..., 0] + 128) >> 8


def tile_lut(h: np.ndarray, clip: int, dark_below: int):
    """(LUT (256,) int64, flag) of one tile from its histogram."""
    h = h.astype(np.int64)
    n = int(h.sum())
    c = np.cumsum(h)
    p99 = int(np.argmax(100 * c >= 99 * n))
    v = np.arange(256, dtype=np.int64)
    if p99 >= dark_below:
        return v, 0
    lim = max(1, (clip * n) >> 16)
    ex = int(np.maximum(h - lim, 0).sum())
    h = np.minimum(h, lim) + ex // 256 + (v < ex % 256)
    c = np.cumsum(h)
    assert c[255] == n
    return np.maximum(v, (2 * 255 * c + n) // (2 * n)), 1


def axis(extent: int, T: int):
    nt = -(-extent // T)
    p = 2 * np.arange(extent, dtype=np.int64) + 1 - T
    q = p // (2 * T)                                      # numpy's floor division
    return np.clip(q, 0, nt - 1), np.clip(q + 1, 0, nt - 1), np.where(p < 0, 0, p % (2 * T))


def luts(frame: np.ndarray, tile=0, clip=0, dark_below=0):
    """(LUTs (ny, nx, 256) int64, flags (ny, nx) int64) of a BGR frame."""
    T, clip, dark_below = resolve(tile, clip, dark_below)
    rows, cols = frame.shape[:2]
    Y = luma(frame)
    ny, nx = -(-rows // T), -(-cols // T)
    L = np.zeros((ny, nx, 256), np.int64)
    F = np.zeros((ny, nx), np.int64)
    for j in range(ny):
        for i in range(nx):
            h = np.bincount(Y[j * T:(j + 1) * T, i * T:(i + 1) * T].ravel(), minlength=256)
            L[j, i], F[j, i] = tile_lut(h, clip, dark_below)
    return L, F


def enhance(frame: np.ndarray, tile=0, clip=0, dark_below=0):
    """(enhanced frame uint8, number of flagged tiles)."""
    T, clip, dark_below = resolve(tile, clip, dark_below)
    rows, cols = frame.shape[:2]
    if rows == 0 or cols == 0:
        return frame.copy(), 0
    L, F = luts(frame, T, clip, dark_below)
    Y = luma(frame)
    D = 2 * T
    j0, j1, wy = (a[:, None] for a in axis(rows, T))
    i0, i1, wx = (a[None, :] for a in axis(cols, T))
    v = (L[j0, i0, Y] * (D - wy) * (D - wx) + L[j0, i1, Y] * (D - wy) * wx + L[j1, i0, Y] * wy * (D - wx) + L[j1, i1, Y] * wy * wx)
    Yn = (2 * v + D * D) // (2 * D * D)
    Yd = np.maximum(Y, 1)
    f = frame.astype(np.int64)
    g = np.minimum(255, (2 * f * Yn[..., None] + Yd[..., None]) // (2 * Yd[..., None]))
    out = np.where((Yn == Y)[..., None], f, g)
    return out.astype(np.uint8), int(F.sum())


# ---------------------------------------------------------------------------------------------- frames the tests share
def apply_gain(frame: np.ndarray, gain) -> np.ndarray:
    """clip(rint(f * g), 0, 255) per pixel on every channel; gain: a scalar or a (rows, cols) / (1, cols) array."""
    g = np.asarray(gain, np.float64)
    if g.ndim == 2:
        g = g[..., None]
    return np.clip(np.rint(frame.astype(np.float64) * g), 0, 255).astype(np.uint8)


def half_dark(frame: np.ndarray, gain: float = 0.04) -> np.ndarray:
    """left half x gain, right half x 1"""
    g = np.ones((1, frame.shape[1]))
    g[:, :frame.shape[1] // 2] = gain
    return apply_gain(frame, g)


def contents(rows: int, cols: int, tile: int = 64):
    """name -> frame: the contents the host and GPU tests run at a shape"""
    rng = np.random.default_rng(rows * 4099 + cols)
    noise = rng.integers(0, 256, (rows, cols, 3), dtype=np.uint8)
    per_tile = np.zeros((rows, cols, 3), np.uint8)
    for j in range(-(-rows // tile)):
        for i in range(-(-cols // tile)):
            per_tile[j * tile:(j + 1) * tile, i * tile:(i + 1) * tile] = (7 * j + 13 * i + 1) % 40
    ramp = np.zeros((rows, cols, 3), np.uint8)
    ramp[...] = ((np.arange(cols)[None, :] * 40 // max(cols, 1) + np.arange(rows)[:, None] % 3) % 48)[..., None]
    ramp[..., 1] //= 2
    y0 = np.zeros((rows, cols, 3), np.uint8)
    y0[..., 0] = 4
    return {
        "black": np.zeros((rows, cols, 3), np.uint8),
        "white": np.full((rows, cols, 3), 255, np.uint8),
        "per_tile": per_tile,
        "ramp": ramp,
        "noise006": apply_gain(noise, 0.06),
        "y0": y0,
        "half": half_dark(noise),
    }
