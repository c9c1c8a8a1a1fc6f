"""CPU: the input noise's rule on its model, tests/noise_model.py -- the Philox known answers, the extremes of
the normal recipe, the moments and independence of a 2^20 block, and the slab layouts against a plain loop over the rule."""
import numpy as np
import pytest

import noise_model as NM

# Random123's kat_vectors for philox4x32 with 10 rounds: ctr / key -> output
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("ctr,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(ctr, key, want):
    got = tuple(int(v) for v in NM.philox4x32_10(*ctr, *key))
    assert got == want, [hex(v) for v in got]


def test_extreme_words_give_finite_normals():
    """the words 0 and ffffffff: u = 2^-24 and 1 - 2^-24, a = 0 and 2 - 2^-23 -- no log(0), |z| <= 5.77"""
    for wa in (0, 0xffffffff):
        for wb in (0, 0xffffffff):
            w = [np.uint64(wa), np.uint64(wb), np.uint64(wa), np.uint64(wb)]
            z, r = NM.normals(w)
            assert np.isfinite(z).all() and np.abs(z).max() <= 5.77, (wa, wb, z)
            u32 = (np.float32(wa >> 9) + np.float32(0.5)) * np.float32(2.0 ** -23)
            assert 0 < float(u32) < 1 and float(u32) == ((wa >> 9) + 0.5) * 2.0 ** -23           # exact in f32
    assert abs(NM.normals([np.uint64(0)] * 4)[1].max() - np.sqrt(48 * np.log(2.0))) < 1e-12      # the largest radius: 5.768


@pytest.fixture(scope="module")
def blocks():
    H, W, n = 128, 256, 32
    base = NM.z_block(H, W, n, 0, 0, 0, 0)
    others = dict(step=NM.z_block(H, W, n, 1, 0, 0, 0), lane=NM.z_block(H, W, n, 0, 1, 0, 0), seed=NM.z_block(H, W, n, 0, 0, 1, 0),
                  draw=NM.z_block(H, W, n, 0, 0, 0, 1))
    return base, others


def test_moments_of_a_2_20_block_within_5_standard_errors(blocks):
    """mean (SE 1/sqrt N), variance (sqrt(2/N)) and fourth moment (E z^8 - 9 = 96: sqrt(96/N)) of N = 2^20 values.  The cap
    of 5 is a condition, not a measurement (the model measures at most 1.3)."""
    a = blocks[0].ravel()
    N = a.size
    assert N == 1 << 20
    figures = dict(mean=a.mean() * N ** .5, var=((a * a).mean() - 1) / (2 / N) ** .5, fourth=((a ** 4).mean() - 3) / (96 / N) ** .5)
    print(figures)
    for k, v in figures.items():
        assert abs(v) <= 5, (k, v)


def test_no_correlation_across_counters_keys_and_neighbours(blocks):
    """the sample correlation with the blocks at step+1, lane+1, seed+1, draw+1 and between neighbours in channel, x and y: each
    within 5 / sqrt(N) (the model measures at most 3.4, at seed+1)"""
    A, others = blocks
    a = A.ravel()
    fig = {k: (a * b.ravel()).mean() * a.size ** .5 for k, b in others.items()}
    for name, (u, v) in dict(channel=(A[:-1], A[1:]), x=(A[:, :, :-1], A[:, :, 1:]), y=(A[:, :-1], A[:, 1:])).items():
        fig[name] = (u * v).mean() * u.size ** .5
    print(fig)
    for k, v in fig.items():
        assert abs(v) <= 5, (k, v)


# ------------------------------------------------------------------------------ layout
H, W, P, B, T = 3, 7, 2, 2, 2
KEY = dict(seed=5, draw=3, step0=4, lane0=6)
# (name, Cx, c0, n, k, sigma): n not a multiple of 4 (the right pair), a zero sigma, every channel folded, an odd start
LAYOUT = [("plain-tail2", 8, 1, 6, 0, (0.5, 0.25, 0.0, 1.0, 2.0, 0.125)), ("folded-thin", 4, 3, 1, 5, (0.5,)),
          ("folded-all", 3, 0, 3, 5, (0.5, 0.0, 0.25)), ("plain-odd", 9, 5, 3, 0, (1.0, 1.0, 1.0)), ("folded-k3-n5", 6, 1, 5, 3, (1.0,) * 5)]


def _case(Cx, c0, n, k, sigma, cyc, bf16, seed=1):
    rng = np.random.default_rng(seed)
    kf = max(k, 1)
    Cxp = (kf * Cx + 15) // 16 * 16
    Hh, Wh = H + 2 * P, W + 2 * P + 3                    # three slack columns
    src = rng.standard_normal((1 + B * T, Cx, H, W)).astype(np.float32)
    src[1, :, 0, 0] = -0.0
    slab = NM.make_slab(rng, src, Hh, Wh, P, Cxp, k, cyc, bf16)
    z = NM.z_images(B, T, n, H, W, **KEY).astype(np.float32)
    got = NM.slab_update(slab, z, 1, Cx, c0, n, sigma, k, cyc, P, H, W)
    return src, slab, z, got, (Hh, Wh, Cxp)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("name,Cx,c0,n,k,sigma", LAYOUT, ids=[c[0] for c in LAYOUT])
def test_vectorised_update_is_the_plain_loop(name, Cx, c0, n, k, sigma, cyc, bf16):
    src, slab, z, got, _ = _case(Cx, c0, n, k, sigma, cyc, bf16)
    want = NM.slab_update_loop(slab, B, T, 1, Cx, c0, n, sigma, k, cyc, P, H, W, **KEY)
    assert got.tobytes() == want.tobytes()
    assert got.tobytes() != slab.tobytes()


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("cyc", [0, 1], ids=["zero-pad", "cyclic"])
@pytest.mark.parametrize("name,Cx,c0,n,k,sigma", LAYOUT, ids=[c[0] for c in LAYOUT])
def test_layout_properties(name, Cx, c0, n, k, sigma, cyc, bf16):
    """image 0 and everything outside the span of the interior pixels keep their bytes; every fold copy equals the plain value of
    the pixel it mirrors; out-of-row copies stay 0 without the wrap and take x' mod W with it; sigma = 0 channels keep their
    bytes (-0.0 included); n % 4 != 0 uses the right pair (the plain value is the rule's own: the loop test above)"""
    src, slab, z, got, (Hh, Wh, Cxp) = _case(Cx, c0, n, k, sigma, cyc, bf16)
    kf = max(k, 1)
    # the plain value of every pixel: the update of a plain slab of the same data
    plain0 = NM.make_slab(np.random.default_rng(2), src, Hh, Wh, P, (Cx + 15) // 16 * 16, 0, 0, bf16)
    plain = NM.slab_update(plain0, z, 1, Cx, c0, n, sigma, 0, 0, P, H, W)
    changed = np.zeros(slab.shape, dtype=bool)
    for kx in range(kf):
        for x in range(W):
            xp = x + kx - kf // 2
            xp = xp % W if cyc else xp
            for o in range(n):
                ch = kx * Cx + c0 + o
                cell = got[1:, P:P + H, P + x, ch]
                if not 0 <= xp < W:
                    assert not cell.any(), (kx, x, "an out-of-row copy stays 0")
                    continue
                assert cell.tobytes() == plain[1:, P:P + H, P + xp, c0 + o].tobytes(), (kx, x, o)
                if sigma[o] != 0:
                    changed[1:, P:P + H, P + x, ch] = True
                else:
                    assert cell.tobytes() == slab[1:, P:P + H, P + x, ch].tobytes()
    raw = lambda a: a.view(np.uint16 if bf16 else np.uint32)
    assert (raw(got)[~changed] == raw(slab)[~changed]).all()
    if sigma[-1] != 0 and not (k and not cyc):
        assert (raw(got)[changed] != raw(slab)[changed]).mean() > 0.9
    # -0.0 under a zero sigma keeps its sign: src[1, :, 0, 0] is -0.0
    for o in range(n):
        if sigma[o] == 0:
            assert raw(got)[1, P, P, (kf // 2) * Cx + c0 + o] == (0x8000 if bf16 else 0x80000000)
