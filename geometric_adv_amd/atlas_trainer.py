"""AtlasNetTrainer (transfer/atlasnet/training: the point-cloud auto-encoder's train_iteration -- model in train mode,
fuse_primitives, chamfer_loss, backward, Adam) on the MI355X: one geoadv_atlas_trainer handle (include/geoadv.h;
csrc/atlas_train.hip) per model.

    tr = AtlasNetTrainer(num_points=2048, batch_size=32, seed=7)       # 25 squares, 2500 template points, fresh weights
    loss = tr.train_step(x)                      # train mode: batch statistics, fresh template points, one Adam step
    recon = tr.eval_model().get_reconstructions(x)   # eval mode through AtlasNetAE on the exported weights
    tr.save('log/atlasnet')                      # network.pth, optimizer.pth, options.json as the reference's trainer

Template points: every step draws number_points // nb_primitives points per primitive, uniform in [0, 1)^2, on the device,
keyed by (seed, training step, primitive, point, coordinate) -- atlas_weights.train_template restates the generator in
numpy.  train_step(x, template=...) takes explicit points of shape (nb_primitives, p, 2).
"""
import numpy as np
import torch

from . import _abi, _lib, atlas_weights as AW
from ._abi import AtlasConfig as _AtlasConfig, AtlasTrainConfig as _AtlasTrainConfig, AtlasWeights as _AtlasWeights
from ._layer_trainer import LayerTrainer, seed64, torch_layer_tensors
from .atlasnet import AtlasNetAE

_STATE = {k: getattr(_abi, "GEOADV_ATLAS_STATE_" + k.upper()) for k in (
    "bn_mean", "bn_var", "running_mean", "running_var", "bn_inv", "bn_shift", "pre_bn", "gmax_row", "template", "latent", "recon",
    "chamfer_idx", "slot1", "slot2")}
_INT_STATES = ("gmax_row", "chamfer_idx")
_PER_LAYER = ("bn_mean", "bn_var", "running_mean", "running_var", "bn_inv", "bn_shift", "pre_bn")
MAX_TRAIN_LAYERS = _abi.GEOADV_ATLAS_ENC_LAYERS + _abi.GEOADV_ATLAS_MAX_DEC_LAYERS      # what geoadv_atlas_trainer_layout writes


def check_batch(batch_size):
    if int(batch_size) < 2:
        raise ValueError("batch_size %d cannot be trained: bn4 and bn5 (after lin1 and lin2) take their statistics over the "
                         "clouds of the batch and need at least 2" % int(batch_size))


def layers(num_layers, decoder_bn):
    """(state-dict prefix with %d for the primitive or None, fan_in, fan_out, conv, BN prefix or None) in
    geoadv_atlas_trainer_layout's order."""
    out = [("encoder." + name, fi, fo, name.startswith("conv"), "encoder.bn%d" % (i + 1), False)
           for i, (name, fi, fo) in enumerate(AW.ENC_LAYERS)]
    for name, fi, fo, bn in AW.dec_layers(num_layers):
        out.append(("decoder.decoder.%d." + name, fi, fo, True, ("decoder.decoder.%d." + bn) if (bn and decoder_bn) else None, True))
    return out


class AtlasNetTrainer(LayerTrainer):
    _PREFIX, _STATE, _INT_STATES = "atlas", _STATE, _INT_STATES
    # counters(): (steps the current optimizer has taken, training steps in all = num_batches_tracked)

    def __init__(self, weights=None, options=None, num_points=2048, batch_size=32, learning_rate=1e-3, seed=0, step=0, slots=None,
                 tracked=None, device=None):
        """weights: {state-dict key: array} (None = atlas_weights.initial_weights(seed) of the options' shape); options: the
        reference's options as far as they apply (nb_primitives, num_layers, remove_all_batchNorms, number_points,
        number_points_eval, template_type; None = the runner's 25 squares of 100 points).  step / slots: the current
        optimizer's steps and Adam's {'exp_avg': {key: array}, 'exp_avg_sq': {key: array}} to continue from (None = fresh);
        tracked: training steps taken in all (num_batches_tracked; None = step)."""
        check_batch(batch_size)
        opt = dict(nb_primitives=25, template_type="SQUARE", number_points=2500)
        opt.update(options or {})
        if weights is not None and "remove_all_batchNorms" not in (options or {}):
            opt["remove_all_batchNorms"] = not AW.has_decoder_bn(AW.strip_prefix(weights))
        opt = AW.options(None, opt)
        opt.setdefault("number_points", 2500)
        shape = AW.check_options(opt)
        self.nb_primitives, self.num_layers = shape["nb_primitives"], shape["num_layers"]
        self.points_per_primitive = int(opt["number_points"]) // self.nb_primitives
        if self.points_per_primitive < 1:
            raise ValueError("number_points %s leaves no template point per primitive" % (opt["number_points"],))
        if weights is None:
            _, weights = AW.initial_weights(seed, self.nb_primitives, self.num_layers, not opt["remove_all_batchNorms"],
                                            int(opt["number_points_eval"]))
        weights = {k: np.asarray(v, np.float32) for k, v in AW.strip_prefix(weights).items() if not k.endswith("num_batches_tracked")}
        self.decoder_bn = AW.validate(weights, self.nb_primitives, self.num_layers, shape["dim_template"])
        opt["remove_all_batchNorms"] = not self.decoder_bn
        self.options = opt
        self.layers = layers(self.num_layers, self.decoder_bn)
        self.param_keys = AW.parameter_names(self.nb_primitives, self.num_layers, self.decoder_bn)
        self.num_points, self.batch_size = int(num_points), int(batch_size)
        self.learning_rate, self.seed = float(learning_rate), int(seed)
        self.device = torch.device(device if device is not None else "cuda:0")
        hw = _AtlasWeights()
        cfg = _AtlasConfig(nb_primitives=self.nb_primitives, points_per_primitive=self.points_per_primitive, dim_template=2,
                           bottleneck_size=AW.BOTTLENECK, hidden_neurons=AW.HIDDEN, num_layers=self.num_layers, activation=0,
                           decoder_bn=int(self.decoder_bn))
        tcfg = _AtlasTrainConfig(self.batch_size, self.num_points, self.points_per_primitive, self.learning_rate, seed64(self.seed),
                                 int(step), int(step if tracked is None else tracked))
        self._open(AW.canonical(weights, self.nb_primitives, self.num_layers), hw, (cfg, hw, tcfg), MAX_TRAIN_LAYERS)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._template = torch.zeros((self.nb_primitives, self.points_per_primitive, 2), dtype=torch.float32, device=self.device)
        if slots is not None:
            self._upload_slots(self._flatten(slots["exp_avg"]), self._flatten(slots["exp_avg_sq"]))

    # ---- device views --------------------------------------------------------------------------------------
    def state(self, what, layer=0, primitive=None):
        """Host copy of what the last step kept (geoadv_atlas_trainer_state).  Layers: 0 .. 4 the encoder's conv1, conv2,
        conv3, lin1, lin2; 5 the decoder's conv1, 6 conv2, 7 ... conv_list.  'bn_mean' / 'bn_var' / 'running_mean' /
        'running_var' / 'bn_inv' / 'bn_shift' (C,) or, for a decoder layer, (nb_primitives, C); 'pre_bn' (rows, C) or
        (nb_primitives, batch * p, C) -- layer 5 gives conv1(template) (nb_primitives, p, 1024), whose sum with the latent
        is that layer's pre-BN activation; 'gmax_row'; 'template'; 'latent'; 'recon'; 'chamfer_idx' 0 / 1; 'slot1';
        'slot2'.  primitive: that primitive's part of a decoder layer's array."""
        a = super().state(what, layer)
        return a[int(primitive)] if primitive is not None and what in _PER_LAYER and int(layer) >= 5 else a

    def _state_shapes(self, layer):
        B, nb, pp = self.batch_size, self.nb_primitives, self.points_per_primitive
        shapes = {"gmax_row": (B, 1024), "template": (nb, pp, 2), "latent": (B, 1024), "recon": (B, nb * pp, 3), "chamfer_idx": (B, -1)}
        C_l = self.layers[layer][2]
        if layer >= 5:                                 # a decoder layer: one row per primitive
            shapes.update(dict.fromkeys(_PER_LAYER, (nb, C_l)), pre_bn=(nb, -1, C_l))
        else:
            shapes["pre_bn"] = (-1, C_l)
        return shapes

    def _tensors(self):
        for l, (pre, fi, fo, conv, bn, dec) in enumerate(self.layers):
            o = self._offsets[4 * l: 4 * l + 4]
            for q in range(self.nb_primitives if dec else 1):
                yield from torch_layer_tensors(pre % q if dec else pre, bn % q if bn and dec else bn, o, fi, fo, conv, q)

    def set_learning_rate(self, learning_rate, reset_optimizer=False):
        """reset_optimizer: a NEW Adam, as the reference builds at its decay epochs (slots and step count start again)."""
        _lib.check(_lib.lib().geoadv_atlas_trainer_set_learning_rate(self._h, float(learning_rate), int(bool(reset_optimizer))),
                   "atlas_trainer_set_learning_rate")
        self.learning_rate = float(learning_rate)

    # ---- the steps -----------------------------------------------------------------------------------------
    def eval_model(self):
        """The AtlasNetAE of the current weights (eval mode: running statistics, the regular template); rebuilt after every
        train_step."""
        if self._eval is None:
            self._eval = AtlasNetAE(state=self.export_state_dict(), options=self.options, batch_size=self.batch_size, device=self.device)
        return self._eval

    def train_step(self, x, template=None):
        """One optimizer step on x (batch_size, num_points, 3): the loss of the pre-update parameters.  template:
        (nb_primitives, p, 2) points, else drawn on the device."""
        x = self._dev(x)
        B, n = self.batch_size, self.num_points
        if tuple(x.shape) != (B, n, 3):
            raise ValueError("train_step takes x (%d, %d, 3); got %s" % (B, n, tuple(x.shape)))
        given = 0
        if template is not None:
            tp = torch.as_tensor(np.asarray(template) if not isinstance(template, torch.Tensor) else template)
            if tuple(tp.shape) != tuple(self._template.shape):
                raise ValueError("template must be of shape %s; got %s" % (tuple(self._template.shape), tuple(tp.shape)))
            self._template.copy_(tp.to(self.device, dtype=torch.float32))
            given = 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().geoadv_atlas_trainer_step(self._h, _lib.ptr(x), given, _lib.ptr(self._template), _lib.ptr(self._loss),
                                                            _lib.stream_handle()), "atlas_trainer_step")
        self._eval = None
        return float(self._loss.cpu().numpy()[0])

    # ---- what the reference's trainer writes ----------------------------------------------------------------
    def export_state_dict(self):
        """{state-dict key: array} of the model: parameters and running statistics (no num_batches_tracked)."""
        out = self.parameters()
        for l, (pre, fi, fo, conv, bn, dec) in enumerate(self.layers):
            if not bn:
                continue
            rm, rv = self.state("running_mean", l), self.state("running_var", l)
            if dec:
                for q in range(self.nb_primitives):
                    out[bn % q + ".running_mean"], out[bn % q + ".running_var"] = rm[q].copy(), rv[q].copy()
            else:
                out[bn + ".running_mean"], out[bn + ".running_var"] = rm, rv
        return out

    def save(self, folder, extra_options=None):
        """network.pth (true num_batches_tracked), optimizer.pth (a torch.optim.Adam state_dict) and options.json."""
        step, tracked = self.counters()
        opt = dict(self.slots(), step=step, lr=self.learning_rate)
        AW.save(folder, dict(self.options, **(extra_options or {})), self.export_state_dict(), optimizer=opt, tracked=tracked)
        return folder

    @classmethod
    def restore(cls, folder, **kwargs):
        """A trainer continuing from a folder `save` (or train_atlasnet, or the reference's trainer) wrote: weights,
        running statistics, num_batches_tracked, Adam's slots, step count and learning rate."""
        options, state, opt, tracked = AW.load_training(folder, kwargs.pop("options", None))
        if opt is None:
            return cls(weights=state, options=options, tracked=tracked, **kwargs)
        kwargs.setdefault("learning_rate", opt["lr"])
        return cls(weights=state, options=options, step=opt["step"], slots=opt, tracked=tracked, **kwargs)
