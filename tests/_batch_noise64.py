"""The noise generator of geoadv_batch_gather (csrc/dataset.hip, file header) restated in numpy: the same 64-bit integer
arithmetic, the same two uniforms, Box-Muller in float64."""
import numpy as np

G = np.uint64(0x9e3779b97f4a7c15)


def mix(z):
    """splitmix64's finaliser on uint64 arrays (wrap-around)."""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def uniforms(seed, counter, slots, n_points):
    """-> (u1 in (0, 1], u2 in [0, 1)), float64 [len(slots), n_points, 3], of the output slots `slots`."""
    with np.errstate(over="ignore"):
        s = np.asarray(slots, dtype=np.uint64)[:, None]
        p = np.arange(n_points, dtype=np.uint64)[None, :]
        key0 = mix(mix(np.uint64(seed) + G) ^ np.uint64(counter))
        key = mix(key0 ^ ((s << np.uint64(32)) | p))
        c = np.arange(1, 4, dtype=np.uint64)
        r = mix(key[:, :, None] + c[None, None, :] * G)
    u1 = ((r >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((r >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normals(seed, counter, slots, n_points):
    """g = sqrt(-2 ln u1) cos(2 pi u2) in float64."""
    u1, u2 = uniforms(seed, counter, slots, n_points)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def noise(g, mu, sigma, clip):
    """mu + clamp(sigma g, -clip, clip) in float64 (clip None or <= 0: no clamp) with the device's fp32 mu, sigma and clip."""
    mu, sigma = float(np.float32(mu)), float(np.float32(sigma))
    d = sigma * g
    if clip is not None and clip > 0:
        d = np.clip(d, -float(np.float32(clip)), float(np.float32(clip)))
    return mu + d
