"""What the entry scripts share: where a run's checkpoints live and how the inference scripts load their models."""
from __future__ import annotations

import os

import numpy as np


def checkpoint_paths(name):
    """(vae_weights, unet_weights, unet_model) under saved_models/, as train_unet.py / train_vae.py write them."""
    unet = os.path.join("saved_models", "unet", name, "unet_weights_" + name + ".best")
    return os.path.join("saved_models", "vae", name, "vae_weights_" + name + ".best.hdf5"), unet + ".hdf5", unet + ".h5"


def load_models(name, d, C, ncond, batch_size, synthetic, seed, want_unet):
    """LatticeDFCVAE (+ AtomUnet) from saved_models/ as the reference loads them; with --synthetic and no checkpoint,
    random weights drawn from np.random seeded with `seed`."""
    from .unet.unet import AtomUnet
    from .vae.lattice_vae import LatticeDFCVAE
    vae_weights, unet_weights, unet_model = checkpoint_paths(name)
    np.random.seed(seed)
    unet = None
    if synthetic and not os.path.exists(unet_model):
        unet = AtomUnet(input_shape=(d, d, d, C), max_batch=batch_size)
        vae = LatticeDFCVAE(input_shape=(d, d, d, C), perceptual_model=unet, cond_shape=ncond)
    else:
        vae = LatticeDFCVAE(input_shape=(d, d, d, C), perceptual_model=unet_model, cond_shape=ncond)
        if want_unet:
            unet = AtomUnet(weights=unet_weights, input_shape=(d, d, d, C), max_batch=batch_size)
    vae._set_model(weights=vae_weights, batch_size=batch_size)
    return vae, unet
