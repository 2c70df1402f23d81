"""Float64 restatement of oess_gray_augment_rgb_f32 (openess_amd/csrc/recon_augment.hip): grey levels -> the
augmented three-channel image of frame2recon.  NumPy only, no torch op in the arithmetic; Philox-4x32-10 and the Box-Muller
transform run on integers and float64, so this is the definition the kernel is held to, not a second fp32 implementation.

Counter layout and uniform mapping (the kernel's header comment states the same):
  key      = (seed & 0xFFFFFFFF, seed >> 32)
  counter  = (g & 0xFFFFFFFF, g >> 32, 0, 0),  g = index of the group of four consecutive elements e = 4 g .. 4 g + 3 of the
             sample's flat [3, H, W] block
  words    = philox4x32_10(counter, key) = (x, y, z, w)
  uniform  = ((word >> 8) + 1) * 2^-24                    24 bits, in (0, 1]
  normals  = element 4 g + 0: r(x) cos(th(y)), + 1: r(x) sin(th(y)), + 2: r(z) cos(th(w)), + 3: r(z) sin(th(w))
             r(a) = sqrt(-2 ln u(a)),  th(b) = 2 pi u(b)
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint64 arrays holding 32-bit words, key: two ints.  Returns the four output words (uint64 arrays < 2^32)."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                 # 32 x 32 -> 64 bits: no overflow in uint64
        hi0, lo0 = p0 >> np.uint64(32), p0 & np.uint64(MASK)
        hi1, lo1 = p1 >> np.uint64(32), p1 & np.uint64(MASK)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def unit24(word):
    """Integer word(s) -> the uniform in (0, 1]; exact in float64 (and in fp32: 24 bits)."""
    return ((np.asarray(word, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24


def noise_words(seed, n_elements):
    """The four Philox words of every element group of a sample with `n_elements` = 3 H W elements: uint64 [groups, 4]."""
    groups = (n_elements + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    zero = np.zeros(groups, dtype=np.uint64)
    seed = int(seed)
    w = philox4x32_10((g & np.uint64(MASK), g >> np.uint64(32), zero, zero), (seed & MASK, seed >> 32))
    return np.stack(w, axis=1)


def normals_from_words(words, dtype=np.float64):
    """Box-Muller on the words of noise_words: [groups, 4] integers -> [groups * 4] normals in `dtype` arithmetic (float64: the
    definition; float32: NumPy's fp32 form of the same expression, the yardstick of the parity bound)."""
    u = unit24(words).astype(dtype)                                          # exact in either type
    two, twopi = dtype(-2.0), dtype(2.0 * np.pi)
    out = np.empty(words.shape, dtype=dtype)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(two * np.log(u[:, a]))
        th = twopi * u[:, b]
        out[:, a] = r * np.cos(th)
        out[:, b] = r * np.sin(th)
    return out.reshape(-1)


def sample_noise(seed, shape, dtype=np.float64):
    """N(0, 1) values of one sample's [3, H, W] block for `seed` (zeros for seed 0)."""
    n = int(np.prod(shape))
    if int(seed) == 0:
        return np.zeros(shape, dtype=dtype)
    return normals_from_words(noise_words(seed, n), dtype)[:n].reshape(shape)


def augment_sample(u8, flip, brightness, contrast, noise_seed, with_noise=True):
    """u8: uint8 [H, W] -> float64 [3, H, W], the steps of K27 in the reference's order (sequence_ov.py:204-221).  brightness
    and contrast are taken as the fp32 factors the kernel receives."""
    b, c = float(np.float32(brightness)), float(np.float32(contrast))
    v = u8.astype(np.float64) / 255.0
    if flip:
        v = v[:, ::-1]
    v = np.clip(b * v, 0.0, 1.0)
    if c != 1.0:
        m = np.mean(0.2989 * v + 0.587 * v + 0.114 * v)
        v = np.clip(c * v + (1.0 - c) * m, 0.0, 1.0)
    out = np.repeat(v[None], 3, axis=0)
    if with_noise and int(noise_seed) != 0:
        out = out + 0.05 * sample_noise(noise_seed, out.shape)
    return out


def augment(u8, flip, brightness, contrast, noise_seed, with_noise=True):
    """uint8 [B, H, W] + per-sample sequences -> float64 [B, 3, H, W]."""
    return np.stack([augment_sample(u8[i], flip[i], brightness[i], contrast[i], noise_seed[i], with_noise) for i in range(u8.shape[0])])
