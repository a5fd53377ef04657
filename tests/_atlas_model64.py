"""An independent float64 model of the AtlasNet auto-encoder (transfer/atlasnet/model/model_blocks.py) for the tests: torch
functional ops (conv1d, batch_norm in eval mode, linear) on the raw state dict in torch's own layouts, template and
primitive fusion written out as the reference does them.  The mistake switches give the variants the tests must tell apart."""
import numpy as np
import torch
import torch.nn.functional as F


def model(state, pc, tmpl, num_layers, swap_template_axes=False, reverse_primitives=False, drop_encoder_bn=False):
    """pc (b, n, 3), tmpl (nb, g2, dim) -> (latent (b, 1024), recon (b, nb * g2, 3)) as float64 numpy."""
    s = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in state.items()
         if not k.endswith("num_batches_tracked")}
    s = {(k[7:] if k.startswith("module.") else k): v for k, v in s.items()}

    def bn(x, k, force=False):
        if (k + ".weight") not in s or (drop_encoder_bn and k.startswith("encoder.") and not force):
            return x
        return F.batch_norm(x, s[k + ".running_mean"], s[k + ".running_var"], s[k + ".weight"], s[k + ".bias"],
                            training=False, eps=1e-5)

    conv = lambda x, k: F.conv1d(x, s[k + ".weight"], s[k + ".bias"])
    with torch.no_grad():
        x = torch.as_tensor(np.asarray(pc), dtype=torch.float64).transpose(1, 2)          # (b, 3, n)
        x = F.relu(bn(conv(x, "encoder.conv1"), "encoder.bn1"))
        x = F.relu(bn(conv(x, "encoder.conv2"), "encoder.bn2"))
        x = bn(conv(x, "encoder.conv3"), "encoder.bn3")
        x, _ = torch.max(x, 2)
        x = F.relu(bn(F.linear(x, s["encoder.lin1.weight"], s["encoder.lin1.bias"]), "encoder.bn4"))
        z = F.relu(bn(F.linear(x, s["encoder.lin2.weight"], s["encoder.lin2.bias"]), "encoder.bn5"))
        nb = len(tmpl)
        prims = []
        for p in range(nb):
            q = nb - 1 - p if reverse_primitives else p
            d = "decoder.decoder.%d." % q
            t = torch.as_tensor(np.array(tmpl[p]), dtype=torch.float64)                    # (g2, dim)
            if swap_template_axes:
                t = t.flip(1)
            t = t.t().unsqueeze(0)                                                         # (1, dim, g2) as get_regular_points
            a = conv(t, d + "conv1") + z.unsqueeze(2)
            a = F.relu(bn(a, d + "bn1"))
            a = F.relu(bn(conv(a, d + "conv2"), d + "bn2"))
            for i in range(num_layers):
                a = F.relu(bn(conv(a, d + "conv_list.%d" % i), d + "bn_list.%d" % i))
            prims.append(conv(a, d + "last_conv").unsqueeze(1))                          # (b, 1, 3, g2)
        out = torch.cat(prims, dim=1)                                                      # (b, nb, 3, g2)
        recon = out.transpose(2, 3).contiguous().view(out.shape[0], -1, 3)                # fuse_primitives
    return z.numpy(), recon.numpy()
