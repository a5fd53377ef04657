"""float64 helpers for the encoder's error tests: the magnitude of the last layer's chain and errors in units of 2^-24 of it.

An fp32 dot product is only as good as the sum of the magnitudes it adds up; an error is measured against that sum, per element,
so that a small latent channel is held to its own chain and not to the largest latent of the batch."""
import numpy as np

U24 = 2.0 ** -24


def last_layer_chain(canon, model, h3):
    """(b, n, C) magnitude of everything the last encoder layer adds up for every point and channel:
    |scale_4| (|h_3| @ |W_4| + |b_4| + |mean_4|) + |beta_4|, with h_3 from the float64 model (oracle.attack_model.AEModel) and
    scale_4 = gamma_4 / sqrt(var_4 + eps).  (mean_4 and beta_4 enter the fp32 shift the epilogue adds.)"""
    mean, beta = (np.abs(np.asarray(canon[k][4], np.float64)) for k in ("mean", "beta"))
    return np.abs(model.scale[4]) * (np.abs(h3) @ np.abs(model.W[4]) + np.abs(model.b[4]) + mean) + beta


def pooled(values, h4):
    """values (b, n, C) at the point the float64 model's max-pool picks per cloud and channel."""
    arg = h4.argmax(axis=1)
    return np.take_along_axis(values, arg[:, None, :], axis=1)[:, 0, :]


def error_units(z, z64, chain_at_pool):
    """|z - z64| in units of 2^-24 of the pooled point's chain."""
    return np.abs(np.asarray(z, np.float64) - z64) / (U24 * np.maximum(chain_at_pool, np.finfo(np.float64).tiny))


def certain_argmax(h4, err):
    """(where the float64 maximum over the points must also be the computed one, float64's argmax) per cloud and channel, for
    computed values within `err` (b, n, C) of h4: the maximum is positive and leads every other point by more than both errors."""
    arg = h4.argmax(axis=1)
    at = lambda v: np.take_along_axis(v, arg[:, None, :], axis=1)[:, 0, :]
    v1, e1 = at(h4), at(err)
    lead = v1[:, None, :] - h4 - err
    np.put_along_axis(lead, arg[:, None, :], np.inf, axis=1)
    return (v1 > 0) & (lead.min(axis=1) > e1), arg
