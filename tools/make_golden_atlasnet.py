"""Writes tests/golden/atlasnet.npz from the REFERENCE's own AtlasNet modules (TEST INFRASTRUCTURE; needs a checkout of the
reference project, run on a host that has one -- never on the GPU machines, where the tests only read the .npz):

    python tools/make_golden_atlasnet.py --reference <checkout of the reference project>

  - transfer/atlasnet/model/model_blocks.py (PointNet, Mapping2Dto3D, Identity) is imported as it is: it needs torch only,
  - SquareTemplate.generate_square is taken from transfer/atlasnet/model/template.py by `ast` (the file imports pymesh at the
    top, so it cannot be imported here),
  - the module tree of model.py / atlasnet.py (EncoderDecoder -> encoder, decoder.decoder[p]) is rebuilt around them, with
    remove_all_batchNorms patching torch.nn.BatchNorm1d after the encoder is built, as atlasnet.py:35-37 does, and wrapped in
    nn.DataParallel for the saved key names (trainer_abstract.py:62-67).

Contents: the seeds and sha256 of the repository's synthetic weights (geometric_adv_amd.atlas_weights.synthetic_state), two
input clouds of 2048 points, latents and reconstructions of two models computed in float64 and stored as float32 (A: 25 x 100
SQUARE, num_layers 2; B: 1 x 2500, num_layers 0, decoder batch norm removed), both models' state-dict key lists, and the
reference's eval-mode template for nb_primitives 1, 3, 4, 25 at number_points_eval 2500.
"""
import argparse
import ast
import hashlib
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from geometric_adv_amd import atlas_weights as AW  # noqa: E402

MODELS = {"a": dict(nb_primitives=25, num_layers=2, decoder_bn=True, seed=11),
          "b": dict(nb_primitives=1, num_layers=0, decoder_bn=False, seed=12)}
TEMPLATE_PRIMS = (1, 3, 4, 25)
CLOUD_SEED = 2024


def weights_sha256(state, nb_primitives, num_layers, decoder_bn):
    h = hashlib.sha256()
    for k in AW.key_names(nb_primitives, num_layers, decoder_bn, prefix=""):
        if not k.endswith("num_batches_tracked"):
            h.update(k.encode())
            h.update(np.ascontiguousarray(state[k], np.float32).tobytes())
    return h.hexdigest()


def clouds():
    return (np.random.default_rng(CLOUD_SEED).random((2, 2048, 3)) - 0.5).astype(np.float32)


def _load_blocks(ref):
    spec = importlib.util.spec_from_file_location("ref_model_blocks",
                                                  os.path.join(ref, "transfer", "atlasnet", "model", "model_blocks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _generate_square(ref):
    path = os.path.join(ref, "transfer", "atlasnet", "model", "template.py")
    tree = ast.parse(open(path).read())
    for cls in tree.body:
        if isinstance(cls, ast.ClassDef) and cls.name == "SquareTemplate":
            for fn in cls.body:
                if isinstance(fn, ast.FunctionDef) and fn.name == "generate_square":
                    fn.decorator_list = []
                    ns = {"np": np}
                    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
                    return ns["generate_square"]
    raise RuntimeError("SquareTemplate.generate_square not found in %s" % path)


def _reference_template(gen, nb_primitives, number_points_eval=2500):
    # Template.get_regular_points (template.py:75-92): generate_square(sqrt(npts)), vertices[:, :2] as float
    vertices, _ = gen(np.sqrt(number_points_eval // nb_primitives))
    return torch.from_numpy(vertices).float()[:, :2].numpy()


def _build(MB, nb_primitives, num_layers, decoder_bn):
    opt = SimpleNamespace(bottleneck_size=1024, dim_template=2, hidden_neurons=512, num_layers=num_layers, activation="relu")

    class Atlasnet(nn.Module):                     # atlasnet.py: the decoders are its only submodule
        def __init__(self):
            super().__init__()
            self.decoder = nn.ModuleList([MB.Mapping2Dto3D(opt) for _ in range(nb_primitives)])

    class EncoderDecoder(nn.Module):               # model.py
        def __init__(self):
            super().__init__()
            self.encoder = MB.PointNet(nlatent=1024)
            saved = torch.nn.BatchNorm1d
            if not decoder_bn:
                torch.nn.BatchNorm1d = MB.Identity  # atlasnet.py:35-37, inside Atlasnet(opt), after PointNet was built
            try:
                self.decoder = Atlasnet()
            finally:
                torch.nn.BatchNorm1d = saved

    return nn.DataParallel(EncoderDecoder())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("GEOADV_REFERENCE"), help="checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "atlasnet.npz"))
    args = ap.parse_args()
    if not args.reference:
        ap.error("--reference (or GEOADV_REFERENCE) is required")
    MB = _load_blocks(args.reference)
    gen = _generate_square(args.reference)
    x = clouds()
    out = {"clouds": x}
    for tag, m in MODELS.items():
        nb, nl, dbn = m["nb_primitives"], m["num_layers"], m["decoder_bn"]
        _, state = AW.synthetic_state(nb, nl, dbn, seed=m["seed"])
        net = _build(MB, nb, nl, dbn)
        keys = list(net.state_dict().keys())
        sd = {k: torch.from_numpy(state[k[len("module."):]]) for k in keys if not k.endswith("num_batches_tracked")}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
        net = net.double().eval()
        tmpl = torch.from_numpy(_reference_template(gen, nb)).double().t().contiguous().unsqueeze(0)     # (1, 2, g2)
        with torch.no_grad():
            latent = net.module.encoder(torch.from_numpy(x).double().transpose(1, 2))
            prims = [net.module.decoder.decoder[p](tmpl, latent.unsqueeze(2)).unsqueeze(1) for p in range(nb)]
            rec = torch.cat(prims, dim=1).transpose(2, 3).contiguous().view(len(x), -1, 3)      # fuse_primitives
        out["latent_" + tag] = latent.numpy().astype(np.float32)
        out["recon_" + tag] = rec.numpy().astype(np.float32)
        out["keys_" + tag] = np.array(keys)
        out["seed_" + tag] = np.int64(m["seed"])
        out["config_" + tag] = np.array([nb, nl, int(dbn)], np.int64)
        out["sha256_" + tag] = np.array(weights_sha256(state, nb, nl, dbn))
    for nb in TEMPLATE_PRIMS:
        out["template_%d" % nb] = _reference_template(gen, nb)
    np.savez_compressed(args.out, **out)
    print("wrote %s (%d bytes)" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
