"""Coreset selection on the MI355X: the kernels against the fp64 restatement (tests/coreset_oracle.py), determinism, short
classes, the reference's picks of fixture g18 end to end, the grade of the features selection uses, and the driver."""
import json
import os

import numpy as np
import pytest
import torch

from tests import coreset_oracle as O

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 93, 150, 700]       # 150: above the LDS-resident size of G~; 700: streamed, and 22 row tiles of the Gram launch


def _pool_features(dim, seed):
    g = torch.Generator().manual_seed(seed)
    # a shared class direction plus noise: features that are not all equidistant from the mean
    f = torch.cat([torch.randn(1, dim, generator=g) * 3 + torch.randn(n, dim, generator=g) * torch.rand(n, 1, generator=g)
                   for n in SIZES]).float()
    offsets = np.concatenate([[0], np.cumsum(SIZES)[:-1]]).tolist()
    return f, offsets


def _compare(kernel, f64, counts, offsets, ipc, method, tag, tol=1e-12):
    """Per class: the kernel's picks equal the oracle's, except at near-ties (relative criterion gap < tol), where the oracle is
    routed on the kernel's pick and the comparison continues.  Returns the number of near-tie differences."""
    ties = 0
    for c, (n, o) in enumerate(zip(counts, offsets)):
        got = kernel[c * ipc:(c + 1) * ipc]
        if n < ipc:
            assert got == [-1] * ipc, (tag, c)
            continue
        rows = [p - o for p in got]
        assert all(0 <= r < n for r in rows), (tag, c, got)
        _, gaps, own = O.select(f64[c], ipc, method, follow=rows)
        for t in range(ipc):
            if own[t] != rows[t]:
                assert gaps[t] < tol, (tag, c, t, own[t], rows[t], gaps[t])
                print("%s class %d step %d: near-tie (gap %.2e) decided %d, oracle %d" % (tag, c, t, gaps[t], rows[t], own[t]))
                ties += 1
    return ties


@pytest.mark.parametrize("dim", [256, 2048, 1000])
def test_kernel_matches_fp64_restatement(dim):
    from video_distillation_amd import coreset
    f, offsets = _pool_features(dim, 100 + dim)
    grams = [O.centred_gram(f[o:o + n].double().numpy()) for n, o in zip(SIZES, offsets)]
    fd = f.cuda()
    for method in ("herding", "k-center"):
        for ipc in (1, 2, 7, 50):
            got = coreset.select(fd, SIZES, offsets, ipc, method, allow_short=True).cpu().tolist()
            _compare(got, grams, SIZES, offsets, ipc, method, "%s D=%d ipc=%d" % (method, dim, ipc))


def test_two_streams_give_bitwise_equal_picks():
    from video_distillation_amd import coreset
    f, offsets = _pool_features(2048, 7)
    fd = f.cuda()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append([coreset.select(fd, SIZES, offsets, 50, m, allow_short=True) for m in ("herding", "k-center")])
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_short_class_marks_only_itself():
    from video_distillation_amd import coreset
    counts, offsets = [5, 3, 6], [0, 5, 8]
    f = torch.randn(14, 300, generator=torch.Generator().manual_seed(9))
    grams = [O.centred_gram(f[o:o + n].double().numpy()) for n, o in zip(counts, offsets)]
    for method in ("herding", "k-center"):
        got = coreset.select(f.cuda(), counts, offsets, 4, method, allow_short=True).cpu().tolist()
        assert got[4:8] == [-1] * 4
        _compare(got, grams, counts, offsets, 4, method, "short " + method)
        with pytest.raises(ValueError):
            coreset.select(f.cuda(), counts, offsets, 4, method)


def _fixture_case(z, gi):
    from oracle import ref_cpu as R
    from video_distillation_amd import distill, utils
    T, H, W = [int(v) for v in z["g%d_shape" % gi]]
    counts = [int(v) for v in z["g%d_counts" % gi]]
    seeds = z["g%d_seeds" % gi]
    clips = torch.cat([torch.randn((n, T, 3, H, W), generator=torch.Generator().manual_seed(int(s))) for n, s in zip(counts, seeds)])
    offsets = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(int).tolist()
    params = R.init_params(int(z["g%d_wseed" % gi]), num_classes=len(counts))
    net = utils.get_network('ConvNet3D', 3, len(counts), (H, W), frames=T, dist=False).cuda()
    net.load_state_dict({k: p.cuda() for k, p in zip(R.PARAM_NAMES, params)})
    for p in net.parameters():
        p.requires_grad = False
    net.eval()
    return distill.RealPool(clips.cuda(), counts, offsets), net, params, counts, offsets


@pytest.mark.parametrize("gi", [0, 1])
def test_build_synset_reproduces_the_reference_picks(golden_dir, gi):
    from video_distillation_amd import coreset
    z = np.load(os.path.join(golden_dir, "g18_coreset.npz"))
    pool, net, _, counts, offsets = _fixture_case(z, gi)
    C = len(counts)
    grams = [z["g%d_gram_%d" % (gi, c)] for c in range(C)]
    ran = 0
    for key in z.files:
        if not key.startswith("g%d_" % gi) or "_ipc" not in key or "error" in key:
            continue
        method, ipc = key[3:].rsplit("_ipc", 1)
        ipc = int(ipc)
        mode = "reference" if method == "k-center" and ipc == 2 else "greedy"
        image_syn, label_syn, index = coreset.build_synset(net, pool, C, ipc, method, kcenter=mode)
        torch.cuda.synchronize()
        got = index.cpu().tolist()
        want = z[key]
        ties = _compare(got, grams, counts, offsets, ipc, method, "g18 geometry %d %s" % (gi, key), tol=1e-5) \
            if mode == "greedy" else 0
        if mode == "reference":
            assert [p - offsets[c] for c in range(C) for p in got[c * ipc:(c + 1) * ipc]] == want.reshape(-1).tolist()
        if ties == 0:
            assert [got[c * ipc + t] - offsets[c] for c in range(C) for t in range(ipc)] == want.reshape(-1).tolist(), key
        assert torch.equal(image_syn, pool.clips[index])
        assert label_syn.tolist() == [c for c in range(C) for _ in range(ipc)]
        ran += 1
    assert ran >= 5


def test_selection_features_are_fp32_grade(golden_dir):
    """Per clip within 1e-5 relative of the fp64 embed; the dithered single-pass ``net.embed`` of the same frozen net is not."""
    from oracle import ref_cpu as R
    from video_distillation_amd import coreset
    z = np.load(os.path.join(golden_dir, "g18_coreset.npz"))
    pool, net, params, counts, offsets = _fixture_case(z, 0)
    feats, cnt, ofs = coreset.class_features(net, pool, list(range(len(counts))))
    want = R.convnet3d_embed(pool.clips.cpu().double(), [p.double() for p in params])
    rel = ((feats.cpu().double() - want).norm(dim=1) / want.norm(dim=1))
    print("class_features per-clip rel-l2: max %.2e" % float(rel.max()))
    assert cnt == counts and ofs == offsets
    assert float(rel.max()) < 1e-5
    with torch.no_grad():
        c = int(np.argmax(counts))
        fe = net.embed(pool.clips[offsets[c]:offsets[c] + counts[c]])
    rel_e = ((fe.cpu().double() - want[offsets[c]:offsets[c] + counts[c]]).norm(dim=1)
             / want[offsets[c]:offsets[c] + counts[c]].norm(dim=1))
    print("net.embed (frozen, no gradient) per-clip rel-l2: max %.2e" % float(rel_e.max()))
    assert float(rel_e.max()) > 1e-5


def test_driver_runs_end_to_end(tmp_path):
    from video_distillation_amd import run_coreset
    g = torch.Generator().manual_seed(21)
    data = tmp_path / "pool.pt"
    torch.save({"clips": torch.randn(12, 8, 3, 64, 64, generator=g), "labels": torch.tensor([2, 0, 1] * 4),
                "test_clips": torch.randn(6, 8, 3, 64, 64, generator=g), "test_labels": torch.tensor([0, 1, 2] * 2)}, data)
    log = tmp_path / "log.jsonl"
    image_syn, label_syn, index = run_coreset.main(["--data_file", str(data), "--frames", "8", "--im_size", "64", "--method",
                                                    "herding", "--ipc", "2", "--epoch_eval_train", "2", "--num_eval", "1",
                                                    "--log_file", str(log)])
    recs = [json.loads(line) for line in open(log)]
    sel = recs[0]
    assert {"picks", "embed_s", "select_s", "method", "ipc"} <= set(sel)
    assert len(sel["picks"]) == 3 and all(len(p) == 2 for p in sel["picks"])
    labels = [2, 0, 1] * 4
    assert all(labels[i] == c for c, p in enumerate(sel["picks"]) for i in p)        # dataset indices of the right class
    assert any("acc_test" in r for r in recs) and any("acc_test_mean" in r and "acc_test_std" in r for r in recs)
    assert tuple(image_syn.shape) == (6, 8, 3, 64, 64) and label_syn.tolist() == [0, 0, 1, 1, 2, 2]
