"""FoldingNetAutoEncoder (transfer/foldingnet/foldingnet_ae.py:27-87) on the MI355X: the FoldingNet auto-encoder the transfer
experiment feeds adversarial clouds to, as one geoadv_fold handle (include/geoadv.h; csrc/foldingnet.hip).  The graph
(prepare_graph.build_graph), both graph pools and the folding decoder all run on the GPU.

    ae = FoldingNetAE('log/foldingnet', epoch=250, seed=7)       # <folder>/checkpoint_250.pth
    recon = ae.get_reconstructions(clouds)                        # float32 (n, 2025, 3)
    loss = ae.get_loss_per_pc(recon, targets)                     # Chamfer per cloud: mean(dist1) + mean(dist2)

Graph_Pooling (foldingnet.py:31-39) keeps 16 of each point's neighbours, drawn with np.random.choice(deg, 16,
replace=False).  The reference never seeds those draws; here a seed is required, and `sampling` says how it is used:
  - 'device': a counter-based generator on the GPU, keyed by (seed, cloud ordinal, pool layer, point)
    (csrc/foldingnet.hip states it exactly).  The ordinal runs on across calls, so a cloud's picks do not depend on
    batch_size or on how the clouds are split between calls -- only on how many clouds the object has seen before it.
  - 'reference': one np.random.RandomState(seed) for the object's lifetime draws every position on the host with
    rs.choice(deg, 16, replace=False), in the reference's order: chunks of 4 clouds (foldingnet_ae.py:46), in each chunk
    pool 1 for every cloud (point by point), then pool 2.  Successive get_reconstructions calls therefore reproduce a run
    of the reference that began with np.random.seed(seed).  The draws cost 13 to 36 ms of host time per cloud of 2048
    points, depending on the CPU (4096 choice calls, each a permutation of the row); the forward itself runs on the GPU
    in any batch size.
"""
import ctypes as C

import numpy as np
import torch

from . import _abi, _lib, fold_weights as FW, ops
from ._abi import FoldWeights as _FoldWeights
from ._model import DeviceModel

G2 = FW.GRID * FW.GRID
K = FW.NUM_NEIGHBOURS
PICKS_GIVEN, PICKS_DEVICE = _abi.GEOADV_FOLD_PICKS_GIVEN, _abi.GEOADV_FOLD_PICKS_DEVICE
REFERENCE_CHUNK = 4
SAMPLINGS = ("device", "reference")


class FoldingNetAE(DeviceModel):
    _destroy = "geoadv_fold_destroy"

    def __init__(self, folder=None, epoch=None, state=None, seed=None, sampling="device", batch_size=32, device=None):
        """Weights from <folder>/checkpoint_<epoch>.pth (fold_weights.load), unless `state` ({key: array}) is given.
        seed (an int) keys the neighbour sampling; sampling is 'device' or 'reference' (see the module docstring).
        batch_size only sets the chunk get_reconstructions feeds the GPU; results do not depend on it."""
        if sampling not in SAMPLINGS:
            raise ValueError("sampling must be one of %s, not %r" % (SAMPLINGS, sampling))
        if seed is None:
            raise ValueError("FoldingNetAE needs a seed: the reference's Graph_Pooling draws neighbours with np.random.choice "
                             "and never seeds it")
        if state is None:
            state = FW.load(folder, epoch)
        else:
            state = {k: v for k, v in FW.strip_prefix(state).items() if not k.endswith("num_batches_tracked")}
            FW.validate(state)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("batch_size must be >= 1")
        self.seed = int(seed)
        self.sampling = sampling
        self.num_points = G2
        self.device = torch.device(device if device is not None else "cuda:0")
        self._rs = np.random.RandomState(self.seed) if sampling == "reference" else None
        self._ordinal = 0                                  # device sampling: clouds seen so far
        self._canon = FW.canonical(state)                  # host arrays alive until create returns
        hw = _FoldWeights()
        for key, arrays in self._canon.items():
            field = getattr(hw, key)
            for i, a in enumerate(arrays):
                field[i] = a.ctypes.data if a is not None else None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_fold_create(C.byref(self._h), C.byref(hw)), "fold_create")

    def graph(self, x):
        """(degree (b, n) int32, knn (b, n, 16) int32, cov (b, n, 9) float32) device tensors of build_graph: the symmetric
        adjacency's row lengths, the 16 nearest neighbours (column 0 of 17 dropped) and their covariance."""
        x = self._as_dev(x)
        b, n = int(x.shape[0]), int(x.shape[1])
        dev = self.device
        deg = torch.empty((b, n), dtype=torch.int32, device=dev)
        knn = torch.empty((b, n, K), dtype=torch.int32, device=dev)
        cov = torch.empty((b, n, 9), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            ws = self._workspace(_lib.lib().geoadv_fold_workspace_bytes(self._h, b, n))
            st = _lib.lib().geoadv_fold_graph(self._h, b, n, _lib.ptr(x), _lib.ptr(deg), _lib.ptr(knn), _lib.ptr(cov),
                                              _lib.ptr(ws), _lib.stream_handle())
        _lib.check(st, "fold_graph")
        return deg, knn, cov

    def forward(self, x, picks=None, seed=None, cloud_offset=0, p1=False):
        """One GPU forward of x (b, n, 3).  With `picks` ((2, b, n, 16) positions in each point's sorted adjacency row,
        pool layer major) the given positions are used; otherwise they are drawn on the device with `seed` (default: the
        object's) and ordinals cloud_offset + k.  Returns a dict of device tensors: code (b, 512), recon (b, 2025, 3),
        picks and cols (2, b, n, 16) int32 -- the positions used and the neighbour indices they resolve to -- and p1
        (b, 2025, 3) if asked for.  Does not advance the object's sampling state."""
        x = self._as_dev(x)
        b, n = int(x.shape[0]), int(x.shape[1])
        dev = self.device
        out = {"code": torch.empty((b, FW.CODE), dtype=torch.float32, device=dev),
               "recon": torch.empty((b, G2, 3), dtype=torch.float32, device=dev),
               "cols": torch.empty((2, b, n, K), dtype=torch.int32, device=dev)}
        if p1:
            out["p1"] = torch.empty((b, G2, 3), dtype=torch.float32, device=dev)
        if picks is not None:
            pk = torch.as_tensor(picks)
            if tuple(pk.shape) != (2, b, n, K):
                raise ValueError("picks must be of shape %s; got %s" % ((2, b, n, K), tuple(pk.shape)))
            pk = pk.to(dev, dtype=torch.int32).contiguous()
            deg = self.graph(x)[0]
            bad = (pk < 0) | (pk >= deg[None, :, :, None])
            if bool(bad.any()):
                l, c, i, t = (int(v) for v in bad.nonzero()[0])
                raise ValueError("picks[%d, %d, %d, %d] = %d is outside [0, %d), the degree of that point"
                                 % (l, c, i, t, int(pk[l, c, i, t]), int(deg[c, i])))
            mode = PICKS_GIVEN
        else:
            pk = torch.empty((2, b, n, K), dtype=torch.int32, device=dev)
            mode = PICKS_DEVICE
        out["picks"] = pk
        s = (self.seed if seed is None else int(seed)) & ((1 << 64) - 1)
        with torch.cuda.device(dev):
            ws = self._workspace(_lib.lib().geoadv_fold_workspace_bytes(self._h, b, n))
            st = _lib.lib().geoadv_fold_forward(self._h, b, n, _lib.ptr(x), mode, s, int(cloud_offset),
                                                _lib.ptr(pk), _lib.ptr(out["cols"]), _lib.ptr(out["code"]),
                                                _lib.ptr(out.get("p1")), _lib.ptr(out["recon"]), _lib.ptr(ws),
                                                _lib.stream_handle())
        _lib.check(st, "fold_forward")
        return out

    def reference_picks(self, degree):
        """Positions (2, b, n, 16) int32 drawn from the object's RandomState in the reference's order (chunks of 4 clouds;
        per chunk pool 1 of every cloud, then pool 2), for host degrees (b, n).  Advances the state."""
        if self._rs is None:
            raise ValueError("reference_picks needs sampling='reference'")
        degree = np.asarray(degree)
        b, n = degree.shape
        out = np.empty((2, b, n, K), np.int32)
        choice = self._rs.choice
        for c0 in range(0, b, REFERENCE_CHUNK):
            for layer in (0, 1):
                for c in range(c0, min(b, c0 + REFERENCE_CHUNK)):
                    dc = degree[c].tolist()
                    oc = out[layer, c]
                    for i in range(n):
                        oc[i] = choice(dc[i], K, replace=False)
        return out

    def restore_model(self, *_args, **_kwargs):
        """foldingnet_ae.py:36-38: the weights are loaded when the object is built."""

    def _forward_batches(self, x, p1=False):
        """Yields (s, e, forward(x[s:e])) over the device clouds x, batch_size at a time, with the object's sampling: device
        draws at ordinals that run on from the clouds seen so far, or reference_picks of all of x drawn first.  Advances
        the sampling state by len(x) once the last batch has been taken."""
        total = int(x.shape[0])
        if total == 0:
            return
        picks = None
        if self.sampling == "reference":
            deg = np.concatenate([self.graph(x[s:s + self.batch_size])[0].cpu().numpy()
                                  for s in range(0, total, self.batch_size)])
            picks = self.reference_picks(deg)
        for s in range(0, total, self.batch_size):
            e = min(total, s + self.batch_size)
            if picks is None:
                r = self.forward(x[s:e], cloud_offset=self._ordinal + s, p1=p1)
            else:
                r = self.forward(x[s:e], picks=picks[:, s:e], p1=p1)
            yield s, e, r
        if picks is None:
            self._ordinal += total

    def get_reconstructions(self, pc_input, flags=None):
        """foldingnet_ae.py:40-66: float32 (n, 2025, 3) reconstructions of any number of clouds, batch_size at a time."""
        x = self._as_dev(pc_input)
        out = np.zeros((int(x.shape[0]), G2, 3), dtype=np.float32)
        for s, e, r in self._forward_batches(x):
            out[s:e] = r["recon"].cpu().numpy()
        return out

    def evaluate(self, clouds, progress=None):
        """tst_foldingnet.py:75-94 per cloud: {'loss_per_pc', 'mid_loss_per_pc'}, float32 (n,) -- the Chamfer distance
        (get_loss_per_pc) between every cloud and its reconstruction, and between it and fold1's output.  The clouds go
        through forward(..., p1=True) batch_size at a time with the sampling and ordinals of get_reconstructions, so a
        fresh object with the same seed reconstructs the same clouds.  The nearest-neighbour distances of all batches are
        kept on the device and averaged per cloud in one step, the one get_loss_per_pc takes over the same clouds, so the
        result equals get_loss_per_pc(get_reconstructions(clouds), clouds) bit for bit and does not depend on batch_size.
        progress(batch index, seconds), if given, is called after every batch, once the GPU has finished it."""
        import time
        x = self._as_dev(clouds)
        total, n = int(x.shape[0]), int(x.shape[1])
        if total == 0:
            return {"loss_per_pc": np.zeros(0, np.float32), "mid_loss_per_pc": np.zeros(0, np.float32)}
        dists = {k: (torch.empty((total, G2), dtype=torch.float32, device=self.device),
                     torch.empty((total, n), dtype=torch.float32, device=self.device)) for k in ("recon", "p1")}
        start = time.time()
        for j, (s, e, r) in enumerate(self._forward_batches(x, p1=True)):
            for k, (to_cloud, to_output) in dists.items():
                to_cloud[s:e], _, to_output[s:e], _ = ops.nn_distance(r[k], x[s:e])
            if progress is not None:
                torch.cuda.synchronize(self.device)
                progress(j, time.time() - start)
                start = time.time()
        return {"loss_per_pc": self._chamfer_per_pc(*dists["recon"]), "mid_loss_per_pc": self._chamfer_per_pc(*dists["p1"])}

    @staticmethod
    def _chamfer_per_pc(d1, d2):
        return (d1.mean(1) + d2.mean(1)).cpu().numpy()

    def get_loss_per_pc(self, pc_recon, target_pc):
        """foldingnet_ae.py:68-87 (ChamferDistance :209-238): per cloud mean(dist1) + mean(dist2) of
        nn_distance(recon, target), as numpy float32."""
        assert len(pc_recon.shape) == 3, 'The pc_input should have 3 dimensions'
        assert len(target_pc.shape) == 3, 'The target_pc should have 3 dimensions'
        assert pc_recon.shape[0] == target_pc.shape[0], 'Number of point clouds must match'
        d1, _, d2, _ = ops.nn_distance(self._as_dev(pc_recon), self._as_dev(target_pc))
        return self._chamfer_per_pc(d1, d2)
