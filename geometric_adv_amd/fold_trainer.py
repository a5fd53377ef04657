"""FoldingNetTrainer (transfer/foldingnet/train_foldingnet.py's model, loss and optimizer step) on the MI355X: one
geoadv_fold_trainer handle (include/geoadv.h; csrc/fold_train.hip) per model.

    tr = FoldingNetTrainer(num_points=2048, batch_size=8, seed=7)
    loss, mid_loss = tr.train_step(x)            # train mode: batch statistics, one torch-form Adam step
    recon = tr.eval_step(x)                      # eval mode through FoldingNetAE on the exported weights
    tr.save('log/foldingnet', 3)                 # checkpoint_3.pth: {'epoch', 'model', 'optimizer'} as the reference's

Neighbour draws: sampling='device' keys the GPU sampler by (seed, cloud ordinal, pool layer, point); the ordinal is the
running count of clouds this trainer has trained on and is stored in the checkpoint ('graph_ordinal').  'reference' draws
np.random.RandomState(seed) positions on the host in the reference's order (FoldingNetAE.reference_picks).  train_step(x,
picks=...) takes explicit positions.
"""
import numpy as np
import torch

from . import _abi, _lib, fold_weights as FW
from ._abi import FoldTrainConfig as _FoldTrainConfig, FoldWeights as _FoldWeights
from ._layer_trainer import LayerTrainer, seed64, torch_layer_tensors
from .foldingnet import FoldingNetAE, PICKS_DEVICE, PICKS_GIVEN, SAMPLINGS, K, G2

_STATE = {k: getattr(_abi, "GEOADV_FOLD_STATE_" + k.upper()) for k in (
    "bn_mean", "bn_var", "running_mean", "running_var", "bn_inv", "bn_shift", "pre_bn", "pool_winner", "gmax_row", "hidden", "picks",
    "cols", "cov", "code", "mid", "recon", "chamfer_idx", "slot1", "slot2")}
_INT_STATES = ("pool_winner", "gmax_row", "picks", "cols", "chamfer_idx")
# (state-dict prefix, fan_in, fan_out, conv, BN index or None) in geoadv_fold_trainer_layout's order
LAYERS = [("encoder." + name, fi, fo, conv, i + 1 if i < 6 else None) for i, (name, fi, fo, conv) in enumerate(FW.ENC_LAYERS)] + \
         [("decoder." + name, fi, fo, True, None) for name, fi, fo in FW.DEC_LAYERS]


def check_batch(batch_size):
    if int(batch_size) < 2:
        raise ValueError("batch_size %d cannot be trained: bn6 (after fc1) takes its statistics over the clouds of the batch "
                         "and needs at least 2" % int(batch_size))


class FoldingNetTrainer(LayerTrainer):
    _PREFIX, _STATE, _INT_STATES = "fold", _STATE, _INT_STATES
    # counters(): (optimizer steps taken, clouds seen)

    def __init__(self, weights=None, num_points=2048, batch_size=8, learning_rate=1e-4, weight_decay=1e-6, seed=0,
                 sampling="device", step=0, slots=None, ordinal=0, device=None):
        """weights: {state-dict key: array} (None = fold_weights.initial_weights(seed)).  step / slots: optimizer steps taken
        and Adam's {'exp_avg': {key: array}, 'exp_avg_sq': {key: array}} to continue from (None = fresh); ordinal: clouds
        seen so far (the device sampler's next ordinal)."""
        check_batch(batch_size)
        if sampling not in SAMPLINGS:
            raise ValueError("sampling must be one of %s, not %r" % (SAMPLINGS, sampling))
        if weights is None:
            weights = FW.initial_weights(seed)
        weights = {k: v for k, v in FW.strip_prefix(weights).items() if not k.endswith("num_batches_tracked")}
        FW.validate(weights)
        self.num_points, self.batch_size = int(num_points), int(batch_size)
        self.learning_rate, self.weight_decay = float(learning_rate), float(weight_decay)
        self.seed, self.sampling = int(seed), sampling
        self.device = torch.device(device if device is not None else "cuda:0")
        self._rs = np.random.RandomState(self.seed) if sampling == "reference" else None
        hw = _FoldWeights()
        cfg = _FoldTrainConfig(self.batch_size, self.num_points, self.learning_rate, self.weight_decay, seed64(self.seed), int(step),
                               int(ordinal))
        self._open(FW.canonical(weights), hw, (hw, cfg), len(LAYERS))
        self._loss = torch.zeros(2, dtype=torch.float32, device=self.device)
        self._picks = torch.zeros((2, self.batch_size, self.num_points, K), dtype=torch.int32, device=self.device)
        self._graph_model = None
        if slots is not None:
            self._upload_slots(self._flatten(slots["exp_avg"]), self._flatten(slots["exp_avg_sq"]))

    def _state_shapes(self, layer):
        """state(what, layer): 'bn_mean' / 'bn_var' / 'running_mean' / 'running_var' / 'bn_inv' / 'bn_shift' / 'pre_bn' of BN
        layer 0 .. 5 (bn1 .. bn6), 'pool_winner' 0 / 1, 'gmax_row', 'hidden' 0 .. 3, 'picks', 'cols', 'cov', 'code', 'mid',
        'recon', 'chamfer_idx' 0 / 1, 'slot1', 'slot2'."""
        B, n = self.batch_size, self.num_points
        return {"pre_bn": (-1, LAYERS[layer][2]), "pool_winner": (B, n, -1), "gmax_row": (B, 1024), "hidden": (-1, 512),
                "picks": (2, B, n, K), "cols": (2, B, n, K), "cov": (B, n, 9), "code": (B, 512), "mid": (B, G2, 3),
                "recon": (B, G2, 3), "chamfer_idx": (B, -1)}

    def _tensors(self):
        for l, (pre, fi, fo, conv, bn) in enumerate(LAYERS):
            yield from torch_layer_tensors(pre, "encoder.bn%d" % bn if bn else None, self._offsets[4 * l: 4 * l + 4], fi, fo, conv)

    # ---- the steps -----------------------------------------------------------------------------------------
    def degrees(self, x):
        """(batch, n) int32 device tensor: the length of every point's adjacency row (what picks index into).  Through a
        FoldingNetAE kept for its graph build alone -- the graph does not depend on the weights, so it is built once."""
        if self._graph_model is None:
            self._graph_model = FoldingNetAE(state=FW.initial_weights(0), seed=self.seed, sampling=self.sampling,
                                             batch_size=self.batch_size, device=self.device)
            self._graph_model._rs = self._rs           # 'reference' sampling: one RandomState for the trainer's lifetime
        return self._graph_model.graph(self._dev(x))[0]

    def eval_model(self):
        """The FoldingNetAE of the current weights (eval mode: running statistics); rebuilt after every train_step."""
        if self._eval is None:
            self._eval = FoldingNetAE(state=self.export_state_dict(), seed=self.seed, sampling=self.sampling,
                                      batch_size=self.batch_size, device=self.device)
        return self._eval

    def train_step(self, x, picks=None):
        """One optimizer step on x (batch_size, num_points, 3): (loss, mid_loss) of the pre-update parameters.  picks:
        (2, batch_size, num_points, 16) positions in each point's sorted adjacency row, else drawn as `sampling` says."""
        x = self._dev(x)
        B, n = self.batch_size, self.num_points
        if tuple(x.shape) != (B, n, 3):
            raise ValueError("train_step takes x (%d, %d, 3); got %s" % (B, n, tuple(x.shape)))
        if picks is None and self.sampling == "reference":
            deg = self.degrees(x).cpu().numpy()
            picks = self._graph_model.reference_picks(deg)
        mode = PICKS_DEVICE
        if picks is not None:
            pk = torch.as_tensor(picks)
            if tuple(pk.shape) != (2, B, n, K):
                raise ValueError("picks must be of shape %s; got %s" % ((2, B, n, K), tuple(pk.shape)))
            pk = pk.to(self.device, dtype=torch.int32).contiguous()
            deg = self.degrees(x)
            if bool(((pk < 0) | (pk >= deg[None, :, :, None])).any()):
                raise ValueError("picks must lie in [0, degree) of their point")
            self._picks.copy_(pk)
            mode = PICKS_GIVEN
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_fold_trainer_step(self._h, _lib.ptr(x), mode, _lib.ptr(self._picks), _lib.ptr(self._loss),
                                                           _lib.ptr(self._loss[1:]), _lib.stream_handle()), "fold_trainer_step")
        self._eval = None
        out = self._loss.cpu().numpy()
        return float(out[0]), float(out[1])

    def eval_step(self, x, picks=None, cloud_offset=0):
        """Eval mode (running statistics) through FoldingNetAE on the exported weights: its forward's dict (code, recon,
        picks, cols)."""
        return self.eval_model().forward(self._dev(x), picks=picks, cloud_offset=cloud_offset)

    # ---- what the reference's torch.save writes --------------------------------------------------------------
    def export_state_dict(self):
        """{state-dict key: array} of the model: parameters and running statistics (no num_batches_tracked)."""
        out = self.parameters()
        for i in range(6):
            out["encoder.bn%d.running_mean" % (i + 1)] = self.state("running_mean", i)
            out["encoder.bn%d.running_var" % (i + 1)] = self.state("running_var", i)
        return out

    def save(self, folder, epoch):
        """checkpoint_<epoch>.pth: {'epoch', 'model', 'optimizer': a torch.optim.Adam state_dict, 'graph_ordinal'}."""
        step, ordinal = self.counters()
        opt = dict(self.slots(), step=step, lr=self.learning_rate, weight_decay=self.weight_decay)
        FW.save(folder, epoch, self.export_state_dict(), optimizer=opt, extra={"graph_ordinal": ordinal})
        return FW.checkpoint_path(folder, epoch)

    @classmethod
    def restore(cls, folder, epoch, **kwargs):
        """A trainer continuing from a checkpoint `save` (or train_foldingnet) wrote: weights, running statistics, Adam's
        slots and step count, and the sampler's cloud ordinal."""
        state, opt, ck = FW.load_training(folder, epoch)
        if opt is None:
            return cls(weights=state, **kwargs)
        return cls(weights=state, step=opt["step"], slots=opt, ordinal=int(ck.get("graph_ordinal", 0)), **kwargs)
