"""Host logic of the gradient-matching driver (``run_dc``) on the CPU with the oracle ops: both kinds of memory on a tiny
``--data_file``, the files it writes, static mode over the golden frame folders, and its flags against the reference parser's."""
import argparse
import os

import numpy as np
import pytest
import torch

from tests.cpu_backend import OracleGMOps
from video_distillation_amd import checkpoint, distill, plan, run_dc, run_s2d

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
C, PER = 2, 3


def _args(tmp_path, *extra):
    return run_dc.build_parser().parse_args([
        "--dataset", "toy", "--Iteration", "1", "--batch_real", "2", "--frames", "8", "--im_size", "64", "--lr_img", "0.1",
        "--save_path", str(tmp_path), "--no_eval"] + list(extra))


def test_images_mode_runs_logs_loss_and_writes_images(tmp_path):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    g = torch.Generator().manual_seed(0)
    clips = torch.randn(C * PER, 8, 3, 64, 64, generator=g)
    labels = torch.tensor([1, 0, 0, 1, 1, 0])
    data = os.path.join(tmp_path, "toy.pt")
    torch.save({"clips": clips, "labels": labels}, data)
    log = []
    tr = run_dc.run(_args(tmp_path, "--memories", "images", "--data_file", data, "--ipc", "1"), ops=OracleGMOps("ours"), log=log)
    losses = [r["Loss"] for r in log if "Loss" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[0] > 0
    assert type(tr) is distill.GMTrainer and (tr.outer_loop, tr.inner_loop) == (1, 1) and tr.steps_done == 2          # get_loops(1)
    got = torch.load(os.path.join(tmp_path, "Baseline_DC", "toy_ipc1_0.1", "images_0.pt"))          # torch.save(image_syn.cpu())
    order = torch.argsort(labels, stable=True)
    assert got.shape == (C, 8, 3, 64, 64) and torch.equal(got, clips[order][[0, PER]])          # --init real, before the first step
    assert not torch.equal(tr.image_syn, got)


def test_static_mode_writes_a_static_memory_run_s2d_accepts(tmp_path):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    g = torch.Generator().manual_seed(1)
    images = torch.randn(C * PER, 3, 64, 64, generator=g)
    labels = torch.tensor([1, 0, 0, 1, 1, 0])
    data = os.path.join(tmp_path, "stills.pt")
    torch.save({"images": images, "labels": labels}, data)
    log = []
    tr = run_dc.run(_args(tmp_path, "--memories", "static", "--data_file", data, "--spc", "2"), ops=OracleGMOps("ours"), log=log)
    losses = [r["Loss"] for r in log if "Loss" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[0] > 0
    assert type(tr) is distill.StillGMTrainer and tr.static.shape == (C * 2, 3, 64, 64) and tr.image_syn.shape == (C * 2, 8, 3, 64, 64)
    path = os.path.join(tmp_path, "Static_DC", "toy_spc2_0.1", "static_0.pt")
    static = checkpoint.load_static(path)
    assert static.shape == (C * 2, 3, 64, 64) and static.dtype == torch.float32
    order = torch.argsort(labels, stable=True)
    assert torch.equal(static, images[order][[0, 1, PER, PER + 1]])          # row c*spc + j = still j of class c (--init real)
    assert torch.equal(torch.load(path)["image"], static)          # the reference's read
    assert not torch.equal(tr.static, static)
    # run_s2d's check of --path_static (run_s2d.py:102-106) takes the file, and refuses it for another spc
    s2d = argparse.Namespace(im_size=64, dpc=2, frames=8, seed=0, path_static=path, spc=2, n_hal=1)
    assert torch.equal(run_s2d.initial_state(s2d, C)[0], static)
    s2d.spc = 10
    with pytest.raises(ValueError, match="holds a static memory of shape"):
        run_s2d.initial_state(s2d, C)
    # a clip file is not a still file, and the other way round
    with pytest.raises(ValueError, match="holds images of shape"):
        run_dc.run(_args(tmp_path, "--memories", "static", "--data_file", data, "--im_size", "32"), ops=OracleGMOps("ours"), log=[])
    clip_file = os.path.join(tmp_path, "clips.pt")
    torch.save({"clips": torch.zeros(2, 8, 3, 64, 64), "labels": torch.tensor([0, 1])}, clip_file)
    with pytest.raises(KeyError, match="images"):
        run_dc.run(_args(tmp_path, "--memories", "static", "--data_file", clip_file), ops=OracleGMOps("ours"), log=[])


def test_save_static_round_trip(tmp_path):
    x = torch.randn(6, 3, 8, 8)
    checkpoint.save_static(str(tmp_path), 7, x, best=True)
    for name in ("static_7.pt", "static_best.pt"):
        assert torch.equal(checkpoint.load_static(os.path.join(tmp_path, name)), x)
    with pytest.raises(ValueError):
        checkpoint.save_static(str(tmp_path), 7, torch.zeros(6, 4, 3, 8, 8))


def test_static_mode_over_the_golden_frame_folders(tmp_path):
    """``singleUCF50`` over tests/golden/frames/UCF101: the pool holds one (3,H,W) image per training video in class order, and
    ``--init real`` takes the first ``spc`` of each class (cyclically where a class has fewer)."""
    from video_distillation_amd import dataset as D
    root = os.path.join(GOLD, "frames")
    args = run_dc.build_parser().parse_args(["--memories", "static", "--dataset", "singleUCF50", "--data_path", root, "--spc", "2",
                                             "--im_size", "112", "--no_eval", "--save_path", str(tmp_path)])
    pool, num_classes, (c_lo, c_hi), loader = run_dc.load_stills(args, 0, 1, torch.device("cpu"))
    dst = D.get_dataset("singleUCF50", root)[6]
    per_class = D.indices_class(dst.labels, 50)
    present = [c for c in range(50) if per_class[c]]
    assert num_classes == 50 and (c_lo, c_hi) == (0, 50) and len(present) >= 2
    assert pool.clips.shape == (len(dst), 3, 112, 112) and pool.counts == [len(per_class[c]) for c in range(50)]
    assert next(iter(loader))[0].dim() == 4          # the test loader yields images; run() wraps it into still clips
    o = 0
    for c in present:          # class order: the rows of class c follow those of every smaller class
        assert pool.offsets[c] == o
        o += pool.counts[c]
    # a present class's --init real rows are its first stills; classes this tiny tree lacks cannot be initialised from data
    mini = distill.RealPool(pool.clips, [pool.counts[c] for c in present], [pool.offsets[c] for c in present])
    tr = distill.StillGMTrainer(OracleGMOps("ours"), mini, plan.NetGeometry(16, 112, 112),
                                len(present), 2, 1, 0.1)
    for k, c in enumerate(present):
        rows = pool.offsets[c] + np.arange(2) % pool.counts[c]
        assert torch.equal(tr.static[2 * k:2 * k + 2], pool.clips[torch.as_tensor(rows)])
    wrapped = run_dc.StillTestLoader(loader, OracleGMOps("ours"), torch.device("cpu"), 4)
    x, y = next(iter(wrapped))
    assert x.shape[1:] == (4, 3, 112, 112) and torch.equal(x[:, 0], x[:, 3]) and len(wrapped) == len(loader) and wrapped.batch_size == 64
    with pytest.raises(ValueError, match="single\\*"):
        args.dataset = "miniUCF101"
        run_dc.load_stills(args, 0, 1, torch.device("cpu"))


# distill_baseline.py:366-415, the names a DC loop reads: (flag, default)
REFERENCE_DEFAULTS = [
    ("dataset", "miniUCF101"), ("method", "DC"), ("model", "ConvNet3D"), ("ipc", 1), ("eval_mode", "S"), ("outer_loop", None),
    ("inner_loop", None), ("num_eval", 5), ("eval_it", 50), ("epoch_eval_train", 1000), ("Iteration", 1000), ("lr_net", 0.001),
    ("lr_img", 1), ("batch_real", 256), ("batch_train", 256), ("init", "real"), ("data_path", "distill_utils/data"),
    ("dis_metric", "ours"), ("num_workers", 8), ("preload", False), ("save_path", "./logged_files"), ("frames", 16),
]


def test_flag_defaults_are_the_reference_parser_s():
    args = run_dc.build_parser().parse_args([])
    for name, default in REFERENCE_DEFAULTS:
        assert getattr(args, name) == default, name
        assert type(getattr(args, name)) is type(default) or name == "lr_img", name
    assert (args.memories, args.spc, args.seed, args.data_file) == ("images", 2, 0, None)
    assert run_dc.build_parser().parse_args(["--preload"]).preload is True
    with pytest.raises(SystemExit):
        run_dc.build_parser().parse_args(["--memories", "s2d"])


def test_unset_loops_come_from_get_loops_and_set_ones_stay(tmp_path):
    g = torch.Generator().manual_seed(2)
    data = os.path.join(tmp_path, "stills.pt")
    torch.save({"images": torch.randn(C * PER, 3, 64, 64, generator=g), "labels": torch.arange(C).repeat_interleave(PER)}, data)
    base = ["--memories", "static", "--data_file", data, "--Iteration", "0", "--init", "noise", "--seed", "3"]
    tr = run_dc.run(_args(tmp_path, *base, "--ipc", "10", "--outer_loop", "1"), ops=OracleGMOps("ours"), log=[])
    assert (tr.outer_loop, tr.inner_loop) == (1, 50)          # the flag, and get_loops(10)[1]; Iteration 0 takes its one step
    noise = torch.randn((C * 2, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    saved = checkpoint.load_static(os.path.join(tmp_path, "Static_DC", "toy_spc2_0.1", "static_0.pt"))
    assert tr.steps_done == 1 and torch.equal(saved, noise) and not torch.equal(tr.static, noise)          # --init noise from --seed
