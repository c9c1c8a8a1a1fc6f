"""CPU model of the input noise (include/nint.h: THE RULE): Philox4x32-10, the normal recipe in f64, and the
slab update in numpy float32 for plain, folded and cyclic layouts -- once vectorised (what the GPU tests compare whole slabs
with) and once as a plain loop over elements that restates the rule word for word (what the vectorised one is checked against).

A slab is a numpy array (images, Hh, Wh, Cxp): float32, or uint16 holding bf16 bits."""
import numpy as np

M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xffffffff)
S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """four arrays of u32 words (held in uint64) for counters that broadcast against each other; key (k0, k1) two ints"""
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xffffffff, (k1 + W1) & 0xffffffff
    return c


def normals(w):
    """four words -> (z, r): z[..., 4] the four normals in f64 (the f64 reference of the f32 recipe), r[..., 4] their radii"""
    zs, rs = [], []
    for a, b in ((w[0], w[1]), (w[2], w[3])):
        u = ((a >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
        ang = (b >> np.uint64(8)).astype(np.float64) * 2.0 ** -23
        r = np.sqrt(-2.0 * np.log(u))
        zs += [r * np.cos(np.pi * ang), r * np.sin(np.pi * ang)]
        rs += [r, r]
    return np.stack(zs, -1), np.stack(rs, -1)


def z_block(H, W, n, step, lane, seed, draw, with_r=False):
    """(n, H, W) f64: the normals of channel offsets [0, n) of every pixel of one image"""
    pix = np.arange(H * W, dtype=np.uint64)[:, None]
    q = np.arange((n + 3) // 4, dtype=np.uint64)[None, :]
    z, r = normals(philox4x32_10(pix, q, int(step) & 0xffffffff, int(lane) & 0xffffffff, seed, draw))   # (HW, Q, 4)
    shape = lambda v: v.reshape(H * W, -1)[:, :n].T.reshape(n, H, W)
    return (shape(z), shape(r)) if with_r else shape(z)


def z_images(B, T, n, H, W, seed=0, draw=0, step0=0, lane0=0, with_r=False):
    """(T*B, n, H, W) f64, image order t*B + b: what nint_noise_normal writes"""
    out = [z_block(H, W, n, step0 + t, lane0 + b, seed, draw, with_r) for t in range(T) for b in range(B)]
    if with_r:
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return np.stack(out)


# ------------------------------------------------------------------------------ storage types
def f32_to_bf16_bits(x):
    """round to nearest even, finite values"""
    u = np.asarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + np.uint64(0x7fff) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.asarray(b, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def noisy(stored_f32, sigma, z_f32):
    """fl32( stored + fl32(sigma * z) ): two float32 operations, never one FMA"""
    prod = (np.float32(sigma) * np.asarray(z_f32, dtype=np.float32)).astype(np.float32)
    return (np.asarray(stored_f32, dtype=np.float32) + prod).astype(np.float32)


def _load(slab, idx):
    v = slab[idx]
    return bf16_bits_to_f32(v) if slab.dtype == np.uint16 else v


def _rounded(slab, v):
    return f32_to_bf16_bits(v) if slab.dtype == np.uint16 else np.asarray(v, dtype=np.float32)


# ------------------------------------------------------------------------------ the slab
def make_slab(rng, src, Hh, Wh, P, Cxp, k, cyc, bf16, junk=True):
    """A slab (N, Hh, Wh, Cxp) that holds `src` (N, Cx, H, W) f32, rounded to the storage type, in the layout the pack entries
    give it -- plain (k = 0), or folded: slab channel kx*Cx + c of pixel x holds channel c of pixel x + kx - k/2 (0 outside the
    row, or that pixel mod W with cyc).  Every other element -- halo rows and columns, slack columns, pad channels -- is junk:
    random bits (`junk`), else 0."""
    N, Cx, H, W = src.shape
    kf = max(k, 1)
    dt = np.uint16 if bf16 else np.float32
    if junk:
        raw = rng.integers(0, 1 << (16 if bf16 else 32), size=(N, Hh, Wh, Cxp), dtype=np.uint64)
        slab = raw.astype(np.uint16) if bf16 else raw.astype(np.uint32).view(np.float32)
    else:
        slab = np.zeros((N, Hh, Wh, Cxp), dtype=dt)
    vals = f32_to_bf16_bits(src) if bf16 else src.astype(np.float32)
    for kx in range(kf):
        for x in range(W):
            xp = x + kx - kf // 2
            if cyc:
                xp %= W
            inside = 0 <= xp < W
            for c in range(Cx):
                slab[:, P:P + H, P + x, kx * Cx + c] = vals[:, c, :, xp] if inside else dt(0)
    return slab


def slab_update(slab, z, x_n0, Cx, c0, n, sigma, k, cyc, P, H, W):
    """nint_input_noise on images [x_n0, x_n0 + len(z)) of a copy of `slab`, with the normals z (images, n, H, W) f32"""
    out = slab.copy()
    kf = max(k, 1)
    xs = np.arange(W)
    for kx in range(kf):
        xp = xs + kx - kf // 2
        if cyc:
            xp = xp % W
        ok = (xp >= 0) & (xp < W)
        xd, xsrc = xs[ok], xp[ok]
        for o in range(n):
            if sigma[o] == 0:
                continue
            ch = kx * Cx + c0 + o
            for i in range(len(z)):
                rows = out[x_n0 + i, P:P + H, :, ch]            # a view (H, Wh)
                idx = (slice(None), P + xd)
                rows[idx] = _rounded(out, noisy(_load(rows, idx), sigma[o], z[i, o][:, xsrc]))
    return out


def slab_update_loop(slab, B, T, x_n0, Cx, c0, n, sigma, k, cyc, P, H, W, seed, draw, step0, lane0):
    """THE RULE, element by element, with its own Philox call per element (f64 normals rounded to f32)"""
    out = slab.copy()
    kf = max(k, 1)
    for t in range(T):
        for b in range(B):
            img = x_n0 + t * B + b
            for y in range(H):
                for x in range(W):
                    for kx in range(kf):
                        xp = x + kx - kf // 2
                        if cyc:
                            xp %= W
                        if not 0 <= xp < W:
                            continue
                        for o in range(n):
                            if sigma[o] == 0:
                                continue
                            w = philox4x32_10(y * W + xp, o // 4, (step0 + t) & 0xffffffff, (lane0 + b) & 0xffffffff, seed, draw)
                            wa, wb = (w[0], w[1]) if o % 4 < 2 else (w[2], w[3])
                            u = (float(int(wa) >> 9) + 0.5) * 2.0 ** -23
                            a = float(int(wb) >> 8) * 2.0 ** -23
                            r = np.sqrt(-2.0 * np.log(u))
                            zz = np.float32(r * (np.cos(np.pi * a) if o % 2 == 0 else np.sin(np.pi * a)))
                            idx = (img, P + y, P + x, kx * Cx + c0 + o)
                            out[idx] = _rounded(out, noisy(_load(out, idx), sigma[o], zz))
    return out


def noisy_input(x, z, c0, sigma, bf16):
    """What the model is shown, on the host: x (B, T, C, H, W) f32 with channels [c0, c0 + n) replaced by
    round_ET( fl32( round_ET(x) + fl32(sigma z) ) ), z (T*B, n, H, W) f32 in image order t*B + b.  The other channels are
    returned as given (the pack entries round them as they always did)."""
    B, T = x.shape[:2]
    out = np.array(x, dtype=np.float32, copy=True)
    rnd = (lambda v: bf16_bits_to_f32(f32_to_bf16_bits(v))) if bf16 else (lambda v: np.asarray(v, dtype=np.float32))
    for o, s in enumerate(sigma):
        if s == 0:
            continue
        zz = z[:, o].reshape(T, B, *z.shape[2:]).transpose(1, 0, 2, 3)
        out[:, :, c0 + o] = rnd(noisy(rnd(out[:, :, c0 + o]), s, zz))
    return out
