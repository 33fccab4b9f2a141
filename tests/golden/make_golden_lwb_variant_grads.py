#!/usr/bin/env python3
"""Generate tests/golden/golden_lwb_variant_grads_v1.npz from the REFERENCE's own generators (authoring container only): the training
forward ``forward(bg, src, tsf, Tst, only_tsf=False)`` and ``backward()`` of AddLWB / AvgLWB (generators/lwb_resunet.py) and
SoftGateAddLWB / SoftGateAvgLWB (generators/lwb_softgate_resunet.py) - reduced-width config at S = 64, ns = 2, nt = 1, seeded weights
and inputs from ipercore_amd.synthetic, flows = the rendered Tst of golden_v1.npz (background = -2), a smooth loss (sum of the mean
squared differences to seeded targets).  Stored per generator: the five outputs sub-sampled [..., ::4, ::4], the loss, and per parameter
the gradient's L2 norm, sum, largest magnitude and a seeded sample of 64 elements.

    python tests/golden/make_golden_lwb_variant_grads.py

The constants and the input / loss / sampling helpers below are what tests/test_lwb_fuse_backward_cpu.py imports to restate the case
on the oracle (no reference needed for that)."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ipercore_amd import synthetic  # noqa: E402

S, NS, NT = 64, 2, 1
NF, NRES, BGF = [64, 64, 128], 2, [64, 64, 128]
NSAMPLE = 64
OUT_NAMES = ("bg", "src_img", "src_mask", "tsf_img", "tsf_mask")


def case_inputs(golden_v1):
    """-> bg (1,1,4,S,S), src (1,ns,6,S,S), tsf (1,nt,6,S,S), Tst (1,nt,ns,S,S,2), the five targets."""
    u = lambda shape, seed, name: torch.tensor(synthetic.uniform_image(shape, seed, name))           # noqa: E731
    bg_in, src_in, tsf_in = u((1, 1, 4, S, S), 10, "bg_inputs"), u((1, NS, 6, S, S), 8, "src_inputs"), u((1, NT, 6, S, S), 9, "tsf_inputs")
    Tst = torch.tensor(golden_v1["render/Tst"]).view(1, NT, NS, S, S, 2)
    tgt = [u(s, 500 + i, "tgt") for i, s in enumerate(((1, 1, 3, S, S), (1, NS, 3, S, S), (1, NS, 1, S, S), (1, NT, 3, S, S), (1, NT, 1, S, S)))]
    return bg_in, src_in, tsf_in, Tst, tgt


def loss_of(outs, tgt):
    return sum(((o - t) ** 2).mean() for o, t in zip(outs, tgt))


def sample_index(numel, i):
    """The seeded sample of parameter number i (order of ``param_names``): min(64, numel) distinct flat indices, ascending."""
    rng = np.random.RandomState(1000 + i)
    return np.sort(rng.choice(numel, size=min(NSAMPLE, numel), replace=False))


def main():
    ref = os.environ.get("LWG_REFERENCE", "/root/reference")
    for m in ("cv2", "torchvision", "neural_renderer"):
        sys.modules.setdefault(m, types.ModuleType(m))
    sys.path.insert(0, ref)
    from iPERCore.models.networks.generators.lwb_resunet import AddLWBGenerator, AvgLWBGenerator
    from iPERCore.models.networks.generators.lwb_softgate_resunet import SoftGateAddLWBGenerator, SoftGateAvgLWBGenerator
    g1 = np.load(os.path.join(ROOT, "tests", "golden", "golden_v1.npz"))
    bg_in, src_in, tsf_in, Tst, tgt = case_inputs(g1)
    out = {}
    for name, cls in (("AddLWB", AddLWBGenerator), ("AvgLWB", AvgLWBGenerator), ("SoftGateAddLWB", SoftGateAddLWBGenerator),
                      ("SoftGateAvgLWB", SoftGateAvgLWBGenerator)):
        G = cls(synthetic.gen_cfg(NF, NRES, BGF), temporal=False).train()
        shapes = {k: tuple(v.shape) for k, v in G.state_dict().items()}
        G.load_state_dict({k: torch.tensor(v) for k, v in synthetic.fill_state_dict(shapes, seed=11).items()}, strict=True)
        outs = G(bg_in, src_in, tsf_in, Tst, only_tsf=False)
        loss = loss_of(outs, tgt)
        loss.backward()
        for oname, o in zip(OUT_NAMES, outs):
            out[f"{name}/out/{oname}"] = o.detach().numpy()[..., ::4, ::4].copy()
        out[f"{name}/loss"] = np.array(loss.item(), dtype=np.float64)
        names = [k for k, _ in G.named_parameters()]
        norms, sums, maxs, samples = [], [], [], np.zeros((len(names), NSAMPLE), dtype=np.float32)
        for i, (k, p) in enumerate(G.named_parameters()):
            assert p.grad is not None, k
            g = p.grad.detach().numpy().reshape(-1)
            g64 = g.astype(np.float64)
            norms.append(np.sqrt((g64 * g64).sum()))
            sums.append(g64.sum())
            maxs.append(np.abs(g64).max())
            idx = sample_index(g.size, i)
            samples[i, :idx.size] = g[idx]
        out[f"{name}/param_names"] = np.array(names)
        out[f"{name}/grad_norm"] = np.array(norms, dtype=np.float64)
        out[f"{name}/grad_sum"] = np.array(sums, dtype=np.float64)
        out[f"{name}/grad_max"] = np.array(maxs, dtype=np.float64)
        out[f"{name}/grad_sample"] = samples
    dst = os.path.join(ROOT, "tests/golden/golden_lwb_variant_grads_v1.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes,", len(out), "entries")


if __name__ == "__main__":
    main()
