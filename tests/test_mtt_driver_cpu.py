"""``run_mtt`` (the MTT branches of distill_baseline.py / distill_s2d_ms.py as a driver) on the CPU with the oracle as compute
backend: the two parsers' defaults, one run per kind of memories (C = 3, 64x64x8, syn_steps 2, iterations 0 and 1, no
evaluation), the files they write and the refusals that come before the loop."""
import math
import os

import pytest
import torch

from tests.cpu_backend import OracleMTTOps
from tests.test_traj_cpu import _random_walk
from video_distillation_amd import checkpoint, run_mtt

C, PER, T, HW = 3, 2, 8, 64
SEED = 4


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("mtt")
    g = torch.Generator().manual_seed(8)
    clips = torch.randn(C * PER, T, 3, HW, HW, generator=g)
    torch.save({"clips": clips, "labels": torch.arange(C).repeat(PER)}, d / "toy.pt")          # classes interleaved
    torch.save({"image": torch.randn(C * 2, 3, HW, HW, generator=g)}, d / "static.pt")
    checkpoint.save_expert_buffer(str(d / "buffers"), _random_walk(g, 2, 3))
    return {"data": str(d / "toy.pt"), "static": str(d / "static.pt"), "buffers": str(d / "buffers"), "dir": d, "clips": clips}


def _argv(files, memories, save, *extra):
    return ["--memories", memories, "--method", "MTT", "--dataset", "toy", "--data_file", files["data"], "--buffer_path",
            files["buffers"], "--save_path", save, "--im_size", str(HW), "--frames", str(T), "--syn_steps", "2", "--expert_epochs", "1",
            "--max_start_epoch", "2", "--Iteration", "1", "--no_eval", "--seed", str(SEED)] + list(extra)


def test_parser_defaults_are_each_script_s_own():
    common = dict(dataset='miniUCF101', method='MTT', model='ConvNet3D', eval_mode='S', num_eval=5, epoch_eval_train=1000,
                  lr_lr=1e-5, train_lr=False, batch_syn=None, batch_train=256, expert_epochs=3, syn_steps=64, max_start_epoch=25,
                  data_path='distill_utils/data', save_path='./logged_files', frames=16, num_workers=8, preload=False,
                  # the project's own
                  data_file=None, im_size=112, num_classes=50, log_file=None, no_eval=False, test_videos='host', eval_ranks='rank0',
                  eval_seed=None, seed=0, expert_store='host', buffer_walk='all', max_files=None, fused_flat='on')
    table = {
        "images": dict(common, memories='images', ipc=1, lr_img=1, init='real', eval_it=50, Iteration=1000, lr_teacher=0.001,
                       buffer_path=None),
        "s2d": dict(common, memories='s2d', vpc=5, spc=10, dpc=1, lr_static=100, lr_dynamic=0.01, lr_hal=0.01, no_train_static=False,
                    path_static=None, n_hal=1, startIt=0, eval_it=100, Iteration=15000, lr_teacher=0.01, buffer_path='./buffers'),
    }
    for memories, want in table.items():
        assert vars(run_mtt.build_parser(memories).parse_args([])) == want, memories
    parse = run_mtt.build_parser("images").parse_args
    for bad in (["--method", "DM"], ["--init", "real-all"], ["--expert_store", "disk"], ["--buffer_walk", "first"], ["--fused_flat", "1"],
                ["--vpc", "1"]):
        with pytest.raises(SystemExit):
            parse(bad)
    a = run_mtt.build_parser("s2d").parse_args(["--memories", "s2d", "--vpc", "1", "--spc", "2", "--dpc", "2", "--lr_dynamic=1e4",
                                                "--lr_hal=1e-3", "--train_lr", "--no_train_static", "--path_static", "s.pt",
                                                "--expert_store", "resident", "--buffer_walk", "reference", "--max_files", "2",
                                                "--fused_flat", "off", "--preload"])
    assert (a.vpc, a.lr_dynamic, a.train_lr, a.expert_store, a.buffer_walk, a.max_files, a.fused_flat) == \
        (1, 1e4, True, "resident", "reference", 2, "off")


def _check_log(log, iterations):
    steps = [r for r in log if "Grand_Loss" in r]
    assert [r["step"] for r in steps] == list(range(iterations))
    for r in steps:
        assert math.isfinite(r["Grand_Loss"]) and r["Grand_Loss"] > 0
        assert 0 <= r["Start_Epoch"] < 2 and r["Grand_Loss/%d" % r["Start_Epoch"]] == r["Grand_Loss"]
    assert not any(k.startswith("Accuracy") for r in log for k in r)
    return steps


def test_images_run_writes_the_reference_s_files(files):
    save = str(files["dir"] / "images")
    args = run_mtt.build_parser("images").parse_args(_argv(files, "images", save, "--ipc", "1", "--lr_img", "100", "--lr_teacher", "0.01",
                                                          "--train_lr", "--lr_lr", "1e-3"))
    log = []
    tr = run_mtt.run(args, ops=OracleMTTOps(), log=log)
    steps = _check_log(log, 2)
    d = os.path.join(save, "Baseline_MTT", "toy_ipc1_100.0")
    assert sorted(os.listdir(d)) == ["images_0.pt"]          # iteration 0 is a multiple of 1000; no evaluation, so no *_best
    start = torch.load(os.path.join(d, "images_0.pt"))
    assert tuple(start.shape) == (C, T, 3, HW, HW)
    # --init real: one training clip of every class, in class order (the file interleaves the classes: item i has class i % C)
    for c in range(C):
        assert any(torch.equal(start[c], files["clips"][i]) for i in range(c, C * PER, C)), c
    assert tuple(tr.image_syn.shape) == tuple(start.shape) and not torch.equal(tr.image_syn, start)          # the clips were trained
    assert tr.steps_done == 2 and tr.batch_syn == C and tr.train_lr
    assert steps[0]["Synthetic_LR"] == pytest.approx(0.01, rel=1e-6)          # syn_lr starts at --lr_teacher ...
    assert steps[1]["Synthetic_LR"] != steps[0]["Synthetic_LR"] and float(tr.syn_lr) >= 0.001          # ... and --train_lr steps it
    assert log[0]["expert_store"] == "host" and log[0]["buffer_walk"] == "all" and log[0]["fused_flat"] is False


def test_s2d_run_writes_the_reference_s_files(files):
    save = str(files["dir"] / "s2d")
    args = run_mtt.build_parser("s2d").parse_args(_argv(files, "s2d", save, "--vpc", "1", "--spc", "2", "--dpc", "2", "--n_hal", "2",
                                                       "--path_static", files["static"], "--lr_static", "0.5", "--lr_dynamic=10.0",
                                                       "--lr_hal=1e-4", "--expert_store", "resident", "--buffer_walk", "reference"))
    log = []
    tr = run_mtt.run(args, ops=OracleMTTOps(), log=log)
    steps = _check_log(log, 2)
    d = os.path.join(save, "S2D_multis_MTT", "toy_ipc1_10.0_0.0001")
    assert sorted(os.listdir(d)) == ["dynamic_0.pt", "hal_0.pt", "images_0.pt"]          # the static memory is trained: images_*
    dyn0 = torch.load(os.path.join(d, "dynamic_0.pt"))
    assert tuple(dyn0.shape) == (C * 2, T, 1, HW, HW)
    assert torch.equal(dyn0, torch.randn(C, 2, T, 1, HW, HW, generator=torch.Generator().manual_seed(SEED)).view(-1, T, 1, HW, HW))
    assert torch.equal(torch.load(os.path.join(d, "images_0.pt")), torch.load(files["static"])["image"])
    pairs = checkpoint.load_hallucinators(os.path.join(d, "hal_0.pt"))
    assert len(pairs) == 2 and tuple(pairs[0][0].shape) == (3, 4, 3, 3, 3)
    assert not torch.equal(tr.dynamic, dyn0) and not torch.equal(tr.hal_w.view(-1), pairs[0][0].view(-1))          # the memories changed
    assert not torch.equal(tr.static, torch.load(files["static"])["image"])
    # without --train_lr (the reference's default) syn_lr stays at --lr_teacher
    assert not tr.train_lr and steps[0]["Synthetic_LR"] == steps[1]["Synthetic_LR"] == pytest.approx(0.01, rel=1e-6)
    assert log[0]["expert_store"] == "resident" and log[0]["buffer_walk"] == "reference"


def test_refusals_come_before_the_loop(files):
    parse = run_mtt.build_parser("images").parse_args
    save = str(files["dir"] / "refused")
    with pytest.raises(ValueError, match=r"--max_start_epoch 3 --expert_epochs 1 reads epoch 3 of trajectories that hold epochs 0\.\.2"):
        run_mtt.run(parse(_argv(files, "images", save, "--max_start_epoch", "3")), ops=OracleMTTOps(), log=[])
    with pytest.raises(ValueError, match="--buffer_path"):
        run_mtt.run(parse(["--data_file", files["data"], "--no_eval"]), ops=OracleMTTOps(), log=[])
    with pytest.raises(AssertionError, match="No buffers detected"):
        run_mtt.run(parse(_argv(files, "images", save, "--buffer_path", str(files["dir"]))), ops=OracleMTTOps(), log=[])
    with pytest.raises(ValueError, match="class 0 has 2 training clips"):
        run_mtt.run(parse(_argv(files, "images", save, "--ipc", "3")), ops=OracleMTTOps(), log=[])
    with pytest.raises(ValueError, match=r"--dpc 1 with --vpc 5 indexes out of range"):
        run_mtt.run(run_mtt.build_parser("s2d").parse_args(_argv(files, "s2d", save)), ops=OracleMTTOps(), log=[])
    assert not os.path.exists(save)
