"""Writes tests/golden/synceval_{A,B}.npz (synceval_ref.CASES): the REFERENCE's classic SyncNet
(eval/syncnet/syncnet.py class S) and calc_pdist (eval/syncnet/syncnet_eval.py) in fp32 on the
CPU, on the seeded weights, frames and audio of tests/synceval_ref.py.

    LATENTSYNC_REFERENCE=<reference checkout> python tests/make_synceval_golden.py

The reference is imported at run time only, with empty stub modules for cv2 and
python_speech_features in sys.modules (neither is used by S or calc_pdist).  The MFCC cannot
come from python_speech_features, which is absent: S is fed the MFCC of
synceval_ref.mfcc_oracle (float64 numpy, the library's definition), and the fixture records that
(mfcc_source).  Weights and inputs are functions of their seeds, so a fixture stores neither: it
holds the state-dict key list, the output of every conv / BN / ReLU stage of both towers (whole
up to 16384 elements, above that its RMS and SUBSAMPLE fixed positions), im_feat, cc_feat,
dists, mean_dists and the three results.  Asserted while generating: every stage's RMS lies in
[0.1, 100], at least 20 % of every ReLU output is non-zero, and the two smallest mean_dists
are further apart than MIN_GAP_OVER_RMS of the RMS of mean_dists (what the model test needs for
its av_offset assertion).  Not collected by pytest.
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
import synceval_ref as R  # noqa: E402

MIN_GAP_OVER_RMS = 0.05


def import_reference():
    ref = os.environ.get("LATENTSYNC_REFERENCE")
    if not ref or not os.path.isdir(ref):
        raise SystemExit("set LATENTSYNC_REFERENCE to a checkout of the reference")
    sys.dont_write_bytecode = True
    for name in ("cv2", "python_speech_features"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(1, ref)
    from eval.syncnet.syncnet import S
    from eval.syncnet.syncnet_eval import calc_pdist
    return S, calc_pdist


def _store(out, label, t, seed):
    flat = t.reshape(-1)
    rms = float(flat.double().pow(2).mean().sqrt())
    alive = float((flat != 0).double().mean())
    assert 0.1 <= rms <= 100.0, (label, rms)
    assert alive >= 0.2, (label, alive)
    out[label + "_shape"] = np.array(t.shape, dtype=np.int64)
    out[label + "_rms"] = np.float64(rms)
    idx = R.subsample_index(flat.numel(), seed)
    if idx is None:
        out[label] = flat.numpy().copy()
    else:
        out[label] = flat[idx].numpy().copy()
        out[label + "_idx"] = idx.numpy().astype(np.int32)
    return rms, alive


@torch.no_grad()
def generate(name, S, calc_pdist):
    c = R.CASES[name]
    net = S().float().eval()
    keys = list(net.state_dict().keys())
    net.load_state_dict(R.case_weights(name), strict=True)
    imtv, mf, lastframe = R.case_network_inputs(name)
    cct = torch.from_numpy(mf.astype(float)).float()[None, None]
    im_in = torch.cat([imtv[:, :, i:i + 5] for i in range(lastframe)], 0)
    cc_in = torch.cat([cct[:, :, :, 4 * i:4 * i + 20] for i in range(lastframe)], 0)
    out = {"keys": np.array(keys), "seed": np.int64(c["seed"]), "mfcc_source": np.array("synceval_ref.mfcc_oracle"),
           "lastframe": np.int64(lastframe)}
    for tower, cnn, fc, x in (("lip", net.netcnnlip, net.netfclip, im_in), ("aud", net.netcnnaud, net.netfcaud, cc_in)):
        h, j = x, 0
        for seq, flatten in ((cnn, False), (fc, True)):
            if flatten:
                h = h.reshape(h.shape[0], -1)
            for mod in seq:
                h = mod(h)
                if isinstance(mod, torch.nn.ReLU):
                    t = h.reshape(h.shape[0], h.shape[1], *h.shape[-2:]) if h.dim() == 5 else h
                    rms, alive = _store(out, f"{tower}_stage_{j}", t.clone(), c["seed"] * 100 + j)
                    print(f"{name} {tower} stage {j}: {tuple(t.shape)} rms {rms:.3f} alive {alive:.2f}")
                    j += 1
        assert j == R.N_STAGES
    im_feat, cc_feat = net.forward_lip(im_in), net.forward_aud(cc_in)
    dists = calc_pdist(im_feat, cc_feat, vshift=c["vshift"])
    mean_dists = torch.mean(torch.stack(dists, 1), 1)
    min_dist, minidx = torch.min(mean_dists, 0)
    av_offset = c["vshift"] - minidx
    conf = torch.median(mean_dists) - min_dist
    srt = mean_dists.sort().values
    rms = float(mean_dists.double().pow(2).mean().sqrt())
    gap = float(srt[1] - srt[0])
    assert gap > MIN_GAP_OVER_RMS * rms, (gap, rms)
    out.update(im_feat=im_feat.numpy(), cc_feat=cc_feat.numpy(), dists=torch.stack(dists, 0).numpy(),
               mean_dists=mean_dists.numpy(), av_offset=np.int64(av_offset.item()), min_dist=np.float64(min_dist.item()),
               conf=np.float64(conf.item()), vshift=np.int64(c["vshift"]))
    path = os.path.join(HERE, "golden", f"synceval_{name}.npz")
    np.savez(path, **out)
    print(name, len(keys), "keys,", os.path.getsize(path), "bytes; av_offset", out["av_offset"], "min_dist",
          out["min_dist"], "conf", out["conf"], "gap / rms", gap / rms)
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    S_, pd_ = import_reference()
    for case in R.CASES:
        generate(case, S_, pd_)
