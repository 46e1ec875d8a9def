"""The cases, value regimes and inputs of the SyncBN tests at 2 to 4 emulated ranks, shared by tests/test_syncbn_host.py
(CPU: the references, the float32 emulation of the two merges, the decision caps of the seeds) and
tests/test_gpu_syncbn.py (ics_op_conv_layer / ics_op_conv_link with ranks = R).  B is the PER-RANK batch; every tensor
with a batch dimension holds R B samples, rank-major.  All shapes are cases of test_gpu_conv_layer.py /
test_gpu_conv_link.py or their next smaller relatives.

path                                                    case (per-rank B, S, channels)                       R
fast reduce / apply kernels, MFMA statistics epilogue   layer fast_64   (2, 8, 16 -> 64), U and V form      2, 3, 4
generic kernels (C % 4 != 0)                            layer generic_6 (2, 4, 16 -> 6)                      2, 3
thin first layer (pad_input, 1 -> 16)                   layer thin_1_16 (2, 8, 1 -> 16)                      2
up-split layer, parity-launch statistics blocks         layer upsplit   (2, 8, [16 | up 32] -> 16)           2
conv_winog                                              layer winog     (4, 4, 64 -> 64)                     2
BwdStat partials + global count                         link same_64_128 (2, 8, 16 -> 64 -> 128) U V         2, 3
                                                        link same_igemm_fold (2, 8, 16 -> 72 -> 32) U        2, 3
up-split dxl launch                                     link up_32_16 (2, 4, 16 -> 32 -> up -> 16) U V       2
launch_pool_presum + global count, both tie rules       link pool_64 (3, 8, 16 -> 64, K 64) U                2, 3
GS_POOL reduce kernels                                  link pool_16 (2, 8, 16 -> 16, K 32) V                2
two gradient sources                                    link pool_skip_64 (2, 8, 16 -> 64, K 64, L [64 | up 128] -> 128) U   2

Regimes of the layer's (the link's P's) output y: the per-channel regimes of conv_layer_ref.regime_params (ratio0, ratio30,
ratio1000, constant, dead, tiny_std, huge -- channel c takes regime c % 7), and the rank-heterogeneous ones of
conv_layer_ref.rank_regimes, which alone make the cross-rank terms of the two merges matter.  Regimes of dout:
conv_layer_ref.rank_dout."""
import functools

import numpy as np

import conv_layer_ref as CR
import conv_link_ref as LR

BOTH, UNET, VAE = ("unet", "vae"), ("unet",), ("vae",)


def layer_case(B, S, src, Cout, forms=UNET, ranks=(2,), pad=False, aff=True):
    return dict(B=B, S=S, src=tuple(src), Cout=Cout, forms=forms, ranks=ranks, pad=pad, aff=aff)


LAYER_CASES = {
    "fast_64": layer_case(2, 8, [(16, 0)], 64, BOTH, (2, 3, 4)),
    "generic_6": layer_case(2, 4, [(16, 0)], 6, UNET, (2, 3)),
    "thin_1_16": layer_case(2, 8, [(1, 0)], 16, UNET, (2,), pad=True, aff=False),
    "upsplit": layer_case(2, 8, [(16, 0), (32, 1)], 16, UNET, (2,)),
    "winog": layer_case(4, 4, [(64, 0)], 64, UNET, (2,)),
}
LAYER_VARIANTS = [(n, f, R) for n, c in LAYER_CASES.items() for f in c["forms"] for R in c["ranks"]]


def link_case(link, forms, B, S, C0, Cp, Ck=0, Cl=0, Cq=0, ties=(1,), ranks=(2,)):
    return dict(link=link, forms=forms, kw=dict(B=B, S=S, C0=C0, Cp=Cp, Ck=Ck, Cl=Cl, Cq=Cq), ties=ties, ranks=ranks)


LINK_CASES = {
    "same_64_128": link_case("same", BOTH, 2, 8, 16, 64, Cl=128, ranks=(2, 3)),
    "same_igemm_fold": link_case("same", UNET, 2, 8, 16, 72, Cl=32, ranks=(2, 3)),
    "up_32_16": link_case("up", BOTH, 2, 4, 16, 32, Cl=16),
    "pool_64": link_case("pool", UNET, 3, 8, 16, 64, Ck=64, ties=(1, 0), ranks=(2, 3)),
    "pool_16": link_case("pool", VAE, 2, 8, 16, 16, Ck=32),
    "pool_skip_64": link_case("pool_skip", UNET, 2, 8, 16, 64, Ck=64, Cl=128, Cq=128),
}
LINK_VARIANTS = [(n, f, t, R) for n, c in LINK_CASES.items() for f in c["forms"] for t in c["ties"] for R in c["ranks"]]

# (regime of y, regime of dout).  None: ordinary values; 0: the seven per-channel regimes of conv_layer_ref.REGIMES, one
# per channel (layers only: a link's P takes "ratio30" / "ratio1000" in every channel, as test_gpu_conv_link.py)
LAYER_REGIMES = [(None, "normal"), (0, "normal"), ("rank_shift50", "normal"), ("rank_const", "mean30"), ("rank_zero", "one_rank"),
                 ("rank_std100", "normal"), (None, "one_rank")]
LINK_REGIMES = [(None, "normal"), ("ratio30", "mean30"), ("ratio1000", "normal"), ("rank_shift50", "normal"),
                ("rank_const", "mean30"), ("rank_zero", "one_rank"), ("rank_std100", "normal")]
NO_CARRIER = ("thin_1_16",)       # one input channel: no carrier for rank_shift50 / rank_const


def layer_regimes(name):
    return [g for g in LAYER_REGIMES if not (name in NO_CARRIER and g[0] in ("rank_shift50", "rank_const"))]


def _seed(table, name):
    return 40 + list(table).index(name)


@functools.lru_cache(maxsize=None)
def layer_data(name, form, R, regime=None, dout_regime="normal", B=None):
    c = LAYER_CASES[name]
    off = regime if (regime is None or regime == 0 or regime in CR.REGIMES) else None
    d = CR.make_case((B or c["B"]) * R, c["S"], c["src"], c["Cout"], 27, form, c["aff"], _seed(LAYER_CASES, name), off)
    if regime in CR.RANK_REGIMES:
        CR.rank_regimes(d, R, regime)
    d["dout"] = CR.rank_dout(d["dout"], R, dout_regime, seed=1)
    return d


@functools.lru_cache(maxsize=None)
def link_data(name, form, R, regime=None, dout_regime="normal", B=None):
    c = LINK_CASES[name]
    kw = dict(c["kw"], B=(B or c["kw"]["B"]) * R)
    p = regime if regime in CR.REGIMES else None
    d = LR.make_link(c["link"], form, seed=_seed(LINK_CASES, name), p_regime=p, **kw)
    if regime in CR.RANK_REGIMES:
        CR.rank_regimes(LR.link_case_view(d), R, regime)
    for k in ("dout", "dout_l"):
        if k in d:
            d[k] = CR.rank_dout(d[k], R, dout_regime, seed=2)
    return d


def rank_slice(a, r, R):
    """rank r's samples of a rank-major tensor"""
    B = a.shape[0] // R
    return a[r * B:(r + 1) * B]
