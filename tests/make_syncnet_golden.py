"""Writes tests/golden/syncnet_{A,B,C}.npz (syncnet_ref.CASES): the REFERENCE StableSyncNet
(latentsync/models/stable_syncnet.py) in fp32 on the CPU, on the seeded weights and inputs
of tests/syncnet_ref.py (case_weights / case_inputs).

    LATENTSYNC_REFERENCE=<reference checkout> python tests/make_syncnet_golden.py

The reference is imported at run time only, with oracle/refshim standing in for diffusers and a
pre-seeded latentsync.utils.util.  Weights and inputs are functions of
their seeds, so a fixture stores neither: it holds the state-dict key list, both embeddings,
the cosine and the output of every down_blocks[i] of both encoders -- whole up to 16384
elements, above that its RMS and SUBSAMPLE fixed positions (syncnet_ref.subsample_index), which
keeps each file under 1 MiB.  Not collected by pytest.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
import syncnet_ref as R  # noqa: E402


def import_reference():
    ref = os.environ.get("LATENTSYNC_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set LATENTSYNC_REFERENCE to a checkout of the reference")
    sys.dont_write_bytecode = True
    sys.path.insert(0, os.path.join(REPO, "oracle", "refshim"))
    sys.path.insert(1, ref)
    util = types.ModuleType("latentsync.utils.util")
    util.zero_rank_log = lambda logger, msg: None
    sys.modules["latentsync.utils.util"] = util
    from latentsync.models.stable_syncnet import StableSyncNet
    return StableSyncNet


@torch.no_grad()
def generate(name, StableSyncNet):
    cfg, _, _, seed = R.CASES[name]
    net = StableSyncNet(cfg).float().eval()
    sd = R.case_weights(name)
    keys = list(net.state_dict().keys())
    net.load_state_dict(sd, strict=True)
    image, audio = R.case_inputs(name)
    out = {"keys": np.array(keys), "seed": np.int64(seed)}
    for enc_name, enc, x in (("visual", net.visual_encoder, image), ("audio", net.audio_encoder, audio)):
        h = enc.conv_in(x)
        for i, blk in enumerate(enc.down_blocks):
            h = blk(h)
            idx = R.subsample_index(h.numel(), seed * 100 + i)
            flat = h.reshape(-1)
            out[f"{enc_name}_block_{i}_shape"] = np.array(h.shape, dtype=np.int64)
            out[f"{enc_name}_block_{i}_rms"] = np.float64(flat.double().pow(2).mean().sqrt())
            if idx is None:
                out[f"{enc_name}_block_{i}"] = flat.numpy().copy()
            else:
                out[f"{enc_name}_block_{i}"] = flat[idx].numpy().copy()
                out[f"{enc_name}_block_{i}_idx"] = idx.numpy().astype(np.int32)
        out[f"{enc_name}_n_blocks"] = np.int64(len(enc.down_blocks))
    v, a = net(image, audio)
    out["vision_embeds"], out["audio_embeds"] = v.numpy(), a.numpy()
    out["cosine"] = torch.nn.functional.cosine_similarity(v, a).numpy()
    path = os.path.join(HERE, "golden", f"syncnet_{name}.npz")
    np.savez(path, **out)
    print(name, len(keys), "keys,", os.path.getsize(path), "bytes, cosine", out["cosine"])


if __name__ == "__main__":
    cls = import_reference()
    for case in R.CASES:
        generate(case, cls)
