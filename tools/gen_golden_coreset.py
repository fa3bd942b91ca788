#!/usr/bin/env python3
"""Generate tests/golden/g18_coreset.npz by RUNNING the reference's distill_coreset.main (herding / k-center baselines).

Runs only where the reference checkout is (VD_REFERENCE, CPU fp32).  The reference's modules are imported unmodified, with
empty stub modules for ``torchvision*`` and ``wandb`` (as tools/gen_golden.py does); inside the imported distill_coreset
module ``get_dataset`` is replaced by seeded clips and ``evaluate_synset`` by a hook that captures ``image_syn`` and stops the
run.  The seeded weights reach the script through ``--pretrained_path`` as a state dict.  Nothing of the reference is written
into the fixture except its outputs (the picks) and the centred Gram of its own net run in
``.double()`` (for the analysis of near-ties).

Stored per geometry ``gK`` (K = 0: 64x64x8, classes of 5/9/7/12 clips; K = 1: 112x112x16, D = 2048, 3 classes of 6/10/8):
  gK_shape (T, H, W), gK_counts, gK_seeds (clips of class c = randn((n_c, T, 3, H, W), Generator().manual_seed(seed_c))),
  gK_wseed (weights = oracle.ref_cpu.init_params(wseed, num_classes=C), identical to torch.manual_seed(wseed); ConvNet3D(...)),
  gK_gram_c (fp64 centred Gram of class c), gK_<method>_ipc<k> ((C, k) picks as within-class indices, selection order),
  gK_kcenter_ipc3_error (the message the reference raised).

Usage:  python tools/gen_golden_coreset.py
"""
import argparse
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True
import numpy as np
import torch

REF = os.environ.get("VD_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "g18_coreset.npz")
GEOMETRIES = [((8, 64, 64), [5, 9, 7, 12], [1801, 1802, 1803, 1804], 11),
              ((16, 112, 112), [6, 10, 8], [1811, 1812, 1813], 12)]


class _Stop(Exception):
    pass


def import_reference():
    for name in ("torchvision", "torchvision.datasets", "torchvision.transforms", "torchvision.utils", "wandb"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
    sys.modules["torchvision"].transforms = sys.modules["torchvision.transforms"]
    sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
    sys.path.insert(0, REF)
    import networks  # noqa
    import distill_coreset  # noqa
    return networks, distill_coreset


def class_clips(shape, counts, seeds):
    T, H, W = shape
    return [torch.randn((n, T, 3, H, W), generator=torch.Generator().manual_seed(int(s))) for n, s in zip(counts, seeds)]


class _Clips:
    def __init__(self, per_class):
        self.items = [(x, c) for c, blk in enumerate(per_class) for x in blk]
        self.labels = [c for _, c in self.items]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def run_reference(dc, shape, clips, weights_path, method, ipc):
    T, H, W = shape
    C = len(clips)
    captured = {}

    def get_dataset(dataset, data_path):
        return 3, (H, W), C, [str(c) for c in range(C)], None, None, _Clips(clips), None, None

    def evaluate_synset(it_eval, net, image_syn, label_syn, testloader, args, **kw):
        captured["image_syn"], captured["label_syn"] = image_syn, label_syn
        raise _Stop()

    dc.get_dataset, dc.evaluate_synset = get_dataset, evaluate_synset
    args = argparse.Namespace(dataset="seeded", method=method, model="ConvNet3D", ipc=ipc, eval_mode="S", num_eval=1,
                              epoch_eval_train=1, lr_net=0.001, batch_train=256, data_path=".", pretrained_path=weights_path,
                              num_workers=0, save_path=".", frames=T, preload=False)
    try:
        dc.main(args)
    except _Stop:
        pass
    # map each image_syn row back to its clip (rows are copies of pool clips)
    picks = np.zeros((C, ipc), dtype=np.int64)
    for c in range(C):
        for t in range(ipc):
            row = captured["image_syn"][c * ipc + t]
            hit = [k for k in range(clips[c].shape[0]) if torch.equal(clips[c][k], row)]
            assert len(hit) == 1, (c, t, hit)
            picks[c, t] = hit[0]
    assert captured["label_syn"].tolist() == [c for c in range(C) for _ in range(ipc)]
    return picks


def main():
    networks, dc = import_reference()
    out = {}
    tmp = tempfile.mkdtemp()
    for gi, (shape, counts, seeds, wseed) in enumerate(GEOMETRIES):
        T, H, W = shape
        C = len(counts)
        torch.manual_seed(wseed)
        net = networks.ConvNet3D(channel=3, num_classes=C, net_width=128, net_depth=3, net_act='relu', net_norm='none',
                                 net_pooling='maxpooling', im_size=(H, W), frames=T)
        wpath = os.path.join(tmp, "w%d.pt" % gi)
        torch.save(net.state_dict(), wpath)
        clips = class_clips(shape, counts, seeds)
        k = "g%d_" % gi
        out[k + "shape"] = np.array(shape)
        out[k + "counts"] = np.array(counts)
        out[k + "seeds"] = np.array(seeds)
        out[k + "wseed"] = np.array(wseed)
        out[k + "param_checksum"] = np.array([float(p.detach().double().sum()) for p in net.parameters()])
        net64 = net.double().eval()
        with torch.no_grad():
            for c in range(C):
                f = net64.embed(clips[c].double())
                f = f - f.mean(0, keepdim=True)
                out[k + "gram_%d" % c] = (f @ f.T).numpy()
        for ipc in sorted({1, 3, min(counts)}):
            out[k + "herding_ipc%d" % ipc] = run_reference(dc, shape, clips, wpath, "herding", ipc)
        for ipc in (1, 2):
            out[k + "k-center_ipc%d" % ipc] = run_reference(dc, shape, clips, wpath, "k-center", ipc)
        try:
            run_reference(dc, shape, clips, wpath, "k-center", 3)
            raise AssertionError("the reference's k-center ran at ipc 3")
        except RuntimeError as e:
            out[k + "kcenter_ipc3_error"] = np.array(str(e))
        print("geometry %s: %s" % (shape, {kk: v.tolist() for kk, v in out.items() if kk.startswith(k) and "ipc" in kk}))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%.1f KB)" % (OUT, os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
