"""sqdiff_kernel through ics_op_sqdiff: the per-sample partial sums of (a - b)^2 that become mse_partial / pm_partial of the
VAE loss (ics_op_vae_loss takes them from there), and the gradient coef * (b - a) it writes or accumulates on the way.
per_sample 4096 / 4100 (multiples of 4: the float4 path when no gradient is asked for), 4099 (scalar path) and 8, cut into
1 / 8 / 16 / 256 blocks: chunks rounded up to a multiple of 4 that run past the end of the sample, and blocks with nothing
to do (their partial must be 0, not whatever the buffer held).

Bounds: the kernel takes the differences in float32 and accumulates their squares in double, so the per-sample sums equal
the fp64 sum of the squared float32 differences to 1e-12 relative (the order of the additions alone); the gradient is
coef * d in float32 bit for bit, and when accumulating g + coef * d with the product rounded first or fused.
Measured on the MI355X: per-sample sums within 2.2e-16 of the fp64 sums; gradients bit-equal.
Run time of this file on the MI355X machine: 0.8 s (49 tests)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PER_SAMPLE = (4096, 4100, 4099, 8)
BLOCKS = (1, 8, 16, 256)


@pytest.mark.parametrize("mode", ("sum_only", "grad", "accumulate"))
@pytest.mark.parametrize("blocks", BLOCKS)
@pytest.mark.parametrize("per", PER_SAMPLE)
def test_sqdiff_matches_fp64_sums(per, blocks, mode):
    from icsg3d_amd import engine as E
    B = 3
    rng = np.random.default_rng(per * 1000 + blocks)
    a = rng.standard_normal((B, per)).astype(np.float32)
    b = (a + rng.standard_normal((B, per)) * rng.choice([1e-3, 1.0, 30.0], (B, 1))).astype(np.float32)
    coef = np.float32(2.0 / per * 0.37)
    g0 = rng.standard_normal((B, per)).astype(np.float32)
    part, g = E.sqdiff(a, b, blocks, coef=coef, grad=mode == "grad", accumulate_into=g0 if mode == "accumulate" else None)
    d = b - a                                                   # float32, as the kernel takes it
    assert d.dtype == np.float32 and part.shape == (B, blocks)
    want = (d.astype(np.float64) ** 2).sum(1)
    got = part.sum(1)
    rel = np.abs(got - want) / want
    print("  per_sample %d blocks %d %s: %.3g" % (per, blocks, mode, rel.max()))
    assert (rel <= 1e-12).all(), rel
    # each block's chunk on its own: chunk = ceil(per / blocks) rounded up to a multiple of 4, clipped at the sample's end
    chunk = (-(-per // blocks) + 3) // 4 * 4
    for k in range(blocks):
        w = (d[:, k * chunk:min((k + 1) * chunk, per)].astype(np.float64) ** 2).sum(1)
        assert (np.abs(part[:, k] - w) <= 1e-12 * np.maximum(w, 1e-300)).all(), (k, part[:, k], w)
    if mode == "sum_only":
        assert g is None
    elif mode == "grad":
        assert np.array_equal(g, coef * d)
    else:
        unfused = g0 + coef * d
        fused = (g0.astype(np.float64) + coef.astype(np.float64) * d.astype(np.float64)).astype(np.float32)
        assert ((g == unfused) | (g == fused)).all()


def test_refusals():
    from icsg3d_amd import engine as E
    from icsg3d_amd._lib import IcsError
    a = np.zeros((2, 8), np.float32)
    with pytest.raises(IcsError, match="blocks_per_sample"):
        E.sqdiff(a, a, 0)
    with pytest.raises(ValueError):
        E.sqdiff(a, a[:, :4], 1)
