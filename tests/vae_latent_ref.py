"""Reference of the DFC-VAE's latent link (ics_op_vae_latent) in plain numpy, from oracle/numpy_ref.py's pieces:

    mulv = h [W_mean | W_lv] + [b_mean | b_lv]          (mu | lv) = mulv          (two Dense layers, lattice_vae.py:183-184)
    z    = mu + exp(lv / 2) eps                           zc = [z | cond]           (numpy_ref.sampling; Concatenate)
    Loss contains beta * mean_b KLD_b, KLD_b = -1/2 sum_j (1 + lv - mu^2 - exp(lv))   (numpy_ref.kld_loss, vae_dfc_loss)
    given dzc = dLoss/dzc (its first `latent` columns are dz; the condition takes no gradient):
    dmu = dz + beta mu / B        dlv = dz eps exp(lv / 2) / 2 - beta (1 - exp(lv)) / (2 B)       dmulv = (dmu | dlv)
    dh, d[W_mean | W_lv], dbias = numpy_ref.dense_bwd(h, [W_mean | W_lv], dmulv)

forward / backward evaluate this in any dtype: float64 is the reference, float32 the yardstick e32 (the error the same
formulas make in float32 numpy on the same inputs, as in tests/test_gpu_conv_layer.py).

The elementwise kernels (sampling_kernel, vae_dz_kernel) are judged PER ELEMENT, on the op's own stored float32 mulv (which
takes the GEMM's rounding out, as the BatchNorm statistics are judged on the op's own y): elementwise() gives, for z, dmu and
dlv, the fp64 value, the float32 value and the floor of the bound -- a number of float32 ulps at the largest operand of the
formula's adds, counted from the formula and the formats alone:
    exp     float32 numpy's exp is documented to 2.52 ulps (its SIMD kernels; 2.35 measured over [-10, 4] in
            tests/test_vae_latent_host.py) -- EXP_ULPS; every other operation rounds once, half an ulp
    z       exp, one product, the add: EXP_ULPS + 1, at max(|mu|, |exp(lv / 2) eps|)
    dmu     beta mu, / B, the add: 1.5, at max(|dz|, |beta mu / B|)
    dlv     dz eps exp(lv / 2) / 2: two inexact products and exp (EXP_ULPS + 1); beta (1 - exp(lv)) / (2 B): exp, the
            subtraction, a product, the division (EXP_ULPS + 1.5) -- at ITS largest operand, beta max(1, exp(lv)) / (2 B):
            where lv ~ 0 the subtraction cancels and the term is known to ulps of 1, not of itself; the add (0.5):
            2 EXP_ULPS + 3, at max(|dz eps exp(lv / 2) / 2|, beta max(1, exp(lv)) / (2 B))
The bound of an element is max(2 e32 of that element, floor)."""
import numpy as np

from oracle import numpy_ref as R

EXP_ULPS = 2.52
Z_FLOOR, DMU_FLOOR, DLV_FLOOR = EXP_ULPS + 1.0, 1.5, 2 * EXP_ULPS + 3.0

# (B, latent, ncond); MAX_BATCH: the case that runs on a handle larger than its batch
CASES = ((1, 1, 1), (3, 20, 3), (2, 100, 1), (5, 256, 10), (2, 33, 7))
MAX_BATCH = {(3, 20, 3): 5}
BETAS = (3e-4, 1e-2, 1.0)
LV_REGIMES = ("small", "spread")


def make_case(B, latent, ncond, lv_regime="small", seed=0):
    """h >= 0 (the encoder's Dense(relu) output), W_mean ~ N(0, 1 / latent).  lv_regime "small": |lv| <~ 0.1, as a Glorot
    initialisation leaves it in every whole-step test; "spread": lv over [-10, 4] (the bias carries it, W_lv only jitters)."""
    rng = np.random.default_rng(7000 + seed)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    c = {"h": f(np.maximum(rng.standard_normal((B, latent)), 0)),
         "w_mean": f(rng.standard_normal((latent, latent)) / np.sqrt(latent)),
         "b_mean": f(0.1 * rng.standard_normal(latent)),
         "eps": f(rng.standard_normal((B, latent))), "cond": f(rng.standard_normal((B, ncond))),
         "dzc": f(rng.standard_normal((B, latent + ncond)))}
    if lv_regime == "small":
        c["w_lv"] = f(0.05 * rng.standard_normal((latent, latent)) / np.sqrt(latent))
        c["b_lv"] = f(0.03 * rng.standard_normal(latent))
    else:
        assert lv_regime == "spread"
        c["w_lv"] = f(0.01 * rng.standard_normal((latent, latent)) / np.sqrt(latent))
        c["b_lv"] = f(rng.permutation(np.linspace(-10.0, 4.0, latent)) if latent > 1 else [-7.0])
    return c


def forward(c, dtype=np.float64):
    h, eps, cond = (np.asarray(c[k], dtype) for k in ("h", "eps", "cond"))
    W = np.concatenate([np.asarray(c["w_mean"], dtype), np.asarray(c["w_lv"], dtype)], 1)
    b = np.concatenate([np.asarray(c["b_mean"], dtype), np.asarray(c["b_lv"], dtype)])
    mulv = R.dense_fwd(h, W, b)
    lat = h.shape[1]
    z = R.sampling(mulv[:, :lat], mulv[:, lat:], eps)
    return {"mulv": mulv, "z": z, "zc": np.concatenate([z, cond], 1), "W": W}


def kl_grad(mu, lv, beta, B):
    """d(beta * mean_b kld_loss) / d(mu, lv), B the batch the mean runs over"""
    beta, half, one = mu.dtype.type(beta), mu.dtype.type(0.5), mu.dtype.type(1)
    return beta * mu / mu.dtype.type(B), beta * (-half) * (one - np.exp(lv)) / mu.dtype.type(B)


def dmulv_from(mulv, eps, dz, beta):
    """(dmu, dlv, the sampling part of dlv) in the dtype of mulv, operation by operation as written above"""
    t = mulv.dtype.type
    lat = mulv.shape[1] // 2
    mu, lv = mulv[:, :lat], mulv[:, lat:]
    kmu, klv = kl_grad(mu, lv, beta, mulv.shape[0])
    a = dz * eps * t(0.5) * np.exp(t(0.5) * lv)
    return dz + kmu, a + klv, a


def backward(f, c, beta, dzc=None, dtype=np.float64):
    lat = f["mulv"].shape[1] // 2
    dzc = np.asarray(c["dzc"] if dzc is None else dzc, dtype)
    dmu, dlv, _ = dmulv_from(f["mulv"], np.asarray(c["eps"], dtype), dzc[:, :lat], beta)
    dmulv = np.concatenate([dmu, dlv], 1)
    dh, dW, db = R.dense_bwd(np.asarray(c["h"], dtype), f["W"], dmulv)
    return {"dmulv": dmulv, "dh": dh, "dw_mean": dW[:, :lat], "dw_lv": dW[:, lat:], "dbias": db}


def reference(c, beta, dzc=None):
    """(fp64 outputs, e32 per tensor): e32 tensor-relative, dbias on the scale max|dmulv| B as the test judges it"""
    beta = float(np.float32(beta))          # as the C ABI carries it
    f64, f32 = forward(c), forward(c, np.float32)
    out = dict(f64, **backward(f64, c, beta, dzc))
    got = dict(f32, **backward(f32, c, beta, dzc, np.float32))
    assert got["dh"].dtype == np.float32 and got["z"].dtype == np.float32
    e32 = {k: tensor_error(k, got[k], out) for k in ("mulv", "dh", "dw_mean", "dw_lv", "dbias")}
    return out, e32


def tensor_error(k, got, ref):
    scale = np.abs(ref[k]).max()
    if k == "dbias":
        scale = np.abs(ref["dmulv"]).max() * ref["dmulv"].shape[0]
    return float(np.abs(np.asarray(got, np.float64) - ref[k]).max() / max(scale, 1e-300))


def _ulp(at):
    return np.spacing(np.maximum(np.abs(at), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def elementwise(mulv32, eps, dz, beta):
    """name -> (fp64 value, bound) per element of z, dmu, dlv, from the float32 mulv the op stored (see the module docstring)"""
    mulv32, eps, dz = (np.ascontiguousarray(v, np.float32) for v in (mulv32, eps, dz))
    B, lat = eps.shape
    beta = float(np.float32(beta))
    m64, e64, d64 = mulv32.astype(np.float64), eps.astype(np.float64), dz.astype(np.float64)
    out = {}
    z64, z32 = R.sampling(m64[:, :lat], m64[:, lat:], e64), R.sampling(mulv32[:, :lat], mulv32[:, lat:], eps)
    t64 = np.exp(0.5 * m64[:, lat:]) * e64
    out["z"] = (z64, np.maximum(2 * np.abs(z32 - z64), Z_FLOOR * _ulp(np.maximum(np.abs(m64[:, :lat]), np.abs(t64)))))
    dmu64, dlv64, a64 = dmulv_from(m64, e64, d64, beta)
    dmu32, dlv32, _ = dmulv_from(mulv32, eps, dz, beta)
    assert dmu32.dtype == np.float32 and dlv32.dtype == np.float32
    kmu = np.abs(beta * m64[:, :lat] / B)
    out["dmu"] = (dmu64, np.maximum(2 * np.abs(dmu32 - dmu64), DMU_FLOOR * _ulp(np.maximum(np.abs(d64), kmu))))
    kop = beta * np.maximum(1.0, np.exp(m64[:, lat:])) / (2 * B)
    out["dlv"] = (dlv64, np.maximum(2 * np.abs(dlv32 - dlv64), DLV_FLOOR * _ulp(np.maximum(np.abs(a64), kop))))
    return out
