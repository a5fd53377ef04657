"""AtlasNetAutoEncoder (transfer/atlasnet/atlasnet_ae.py:27-82) on the MI355X: the AtlasNet auto-encoder the transfer
experiment feeds adversarial clouds to, as one geoadv_atlas handle (include/geoadv.h; csrc/atlasnet.hip).

    ae = AtlasNetAE('log/atlasnet_ae')                  # <folder>/network.pth + <folder>/options.json
    recon = ae.get_reconstructions(clouds)            # float32 (n, P, 3), P = nb_primitives * g * g
    loss = ae.get_loss_per_pc(recon, targets)         # Chamfer per cloud: mean(dist1) + mean(dist2)
    latent, recon = ae.forward(device_tensor)         # on the GPU

The input clouds are used raw, as the reference's custom data path does (dataset_shapenet.py:132-143, 230-233: no
normalisation, no resampling).  Unlike the reference (a fixed 2500-point buffer), any P and any number of clouds work.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, atlas_weights as AW, ops
from ._abi import AtlasConfig as _AtlasConfig, AtlasWeights as _AtlasWeights
from ._model import DeviceModel


class AtlasNetAE(DeviceModel):
    _destroy = "geoadv_atlas_destroy"

    def __init__(self, transfer_ae_folder=None, options=None, state=None, batch_size=32, device=None):
        """Weights and options from <transfer_ae_folder>/network.pth and options.json (atlas_weights.load), unless
        `state` (a {key: array} dict without the `module.` prefix) and `options` are given.  batch_size only sets the chunk
        get_reconstructions feeds (the reference's batch_size_test, 32); results do not depend on it."""
        if state is None:
            options, state = AW.load(transfer_ae_folder, options)
        else:
            options = AW.options(None, options)
            state = {k: v for k, v in AW.strip_prefix(state).items() if not k.endswith("num_batches_tracked")}
        shape = AW.check_options(options)
        self.decoder_bn = AW.validate(state, shape["nb_primitives"], shape["num_layers"], shape["dim_template"])
        self.options = options
        self.nb_primitives = shape["nb_primitives"]
        self.num_layers = shape["num_layers"]
        self.grain = shape["grain"]
        self.num_points = self.nb_primitives * self.grain * self.grain       # P, the reconstruction's point count
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.device = torch.device(device if device is not None else "cuda:0")
        self.template = AW.template(self.nb_primitives, self.grain)
        self._canon = AW.canonical(state, self.nb_primitives, self.num_layers)    # host arrays alive until create returns
        cfg = _AtlasConfig(nb_primitives=self.nb_primitives, points_per_primitive=self.grain * self.grain,
                           dim_template=shape["dim_template"], bottleneck_size=AW.BOTTLENECK, hidden_neurons=AW.HIDDEN,
                           num_layers=self.num_layers, activation=0, decoder_bn=int(self.decoder_bn))
        hw = _AtlasWeights()
        for key, arrays in self._canon.items():
            field = getattr(hw, key)
            for i, a in enumerate(arrays):
                field[i] = a.ctypes.data if a is not None else None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_atlas_create(C.byref(self._h), C.byref(cfg), C.byref(hw),
                                                      self.template.ctypes.data), "atlas_create")

    def forward(self, x):
        """(latent (b, 1024), recon (b, P, 3)) float32 device tensors of EncoderDecoder.forward(x, train=False), fused
        primitive-major (fuse_primitives), one call."""
        x = self._as_dev(x)
        b, n = int(x.shape[0]), int(x.shape[1])
        dev = self.device
        latent = torch.empty((b, AW.BOTTLENECK), dtype=torch.float32, device=dev)
        recon = torch.empty((b, self.num_points, 3), dtype=torch.float32, device=dev)
        if b == 0:
            return latent, recon
        L = _lib.lib()
        with torch.cuda.device(dev):
            ws = self._workspace(L.geoadv_atlas_workspace_bytes(self._h, b, n))
            st = L.geoadv_atlas_forward(self._h, b, n, _lib.ptr(x), _lib.ptr(latent), _lib.ptr(recon), _lib.ptr(ws),
                                        _lib.stream_handle())
        _lib.check(st, "atlas_forward")
        return latent, recon

    def restore_model(self, *_args, **_kwargs):
        """atlasnet_ae.py:37-39: degenerate in the reference too (the weights are loaded when the object is built)."""

    def get_reconstructions(self, pc_input, *_flags):
        """atlasnet_ae.py:41-61: float32 (n, P, 3) reconstructions of any number of clouds, batch_size at a time."""
        x = self._as_dev(pc_input)
        out = np.zeros((int(x.shape[0]), self.num_points, 3), dtype=np.float32)
        for s in range(0, int(x.shape[0]), self.batch_size):
            out[s:s + self.batch_size] = self.forward(x[s:s + self.batch_size])[1].cpu().numpy()
        return out

    def get_loss_per_pc(self, pc_recon, target_pc):
        """atlasnet_ae.py:63-82: per cloud mean(dist1) + mean(dist2) of nn_distance(recon, target), as numpy float32."""
        assert len(pc_recon.shape) == 3, 'The pc_input should have 3 dimensions'
        assert len(target_pc.shape) == 3, 'The target_pc should have 3 dimensions'
        assert pc_recon.shape[0] == target_pc.shape[0], 'Number of point clouds must match'
        d1, _, d2, _ = ops.nn_distance(self._as_dev(pc_recon), self._as_dev(target_pc))
        return (d1.mean(1) + d2.mean(1)).cpu().numpy()
