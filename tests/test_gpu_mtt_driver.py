"""``run_mtt`` end to end on the GPU: both kinds of memories with the tiny settings of tests/test_mtt_driver_cpu.py, the expert
store resident and the fused chain on (the driver's defaults for the chain), and one run with evaluation on."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

C, PER, T, HW = 3, 2, 8, 64
SEED = 4


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from tests.test_traj_cpu import _random_walk
    from video_distillation_amd import checkpoint
    d = tmp_path_factory.mktemp("mtt_gpu")
    g = torch.Generator().manual_seed(8)
    clips = torch.randn(C * PER, T, 3, HW, HW, generator=g)
    # six test clips that are ONE clip under the labels 0 0 1 1 2 2: whatever a network answers, it is right twice in six, so
    # the first evaluation is a new best (accuracy 1/3 > 0) whatever its seed
    test_clips = clips[:1].expand(6, -1, -1, -1, -1).contiguous()
    torch.save({"clips": clips, "labels": torch.arange(C).repeat(PER), "test_clips": test_clips,
                "test_labels": torch.arange(C).repeat_interleave(2)}, d / "toy.pt")
    torch.save({"image": torch.randn(C * 2, 3, HW, HW, generator=g)}, d / "static.pt")
    checkpoint.save_expert_buffer(str(d / "buffers"), _random_walk(g, 2, 3))
    return {"data": str(d / "toy.pt"), "static": str(d / "static.pt"), "buffers": str(d / "buffers"), "dir": d}


def _argv(files, memories, save, *extra):
    return ["--memories", memories, "--method", "MTT", "--dataset", "toy", "--data_file", files["data"], "--buffer_path",
            files["buffers"], "--save_path", save, "--im_size", str(HW), "--frames", str(T), "--syn_steps", "2", "--expert_epochs", "1",
            "--max_start_epoch", "2", "--Iteration", "1", "--seed", str(SEED), "--expert_store", "resident"] + list(extra)


def _steps(log, iterations):
    steps = [r for r in log if "Grand_Loss" in r]
    assert [r["step"] for r in steps] == list(range(iterations))
    for r in steps:
        assert math.isfinite(r["Grand_Loss"]) and r["Grand_Loss"] > 0 and 0 <= r["Start_Epoch"] < 2
        assert r["Grand_Loss/%d" % r["Start_Epoch"]] == r["Grand_Loss"]
    assert log[0]["expert_store"] == "resident" and log[0]["fused_flat"] is True
    return steps


def test_images_run_on_the_gpu(files):
    from video_distillation_amd import run_mtt
    save = str(files["dir"] / "images")
    args = run_mtt.build_parser("images").parse_args(_argv(files, "images", save, "--no_eval", "--lr_img", "100", "--lr_teacher", "0.01",
                                                          "--train_lr", "--lr_lr", "1e-3"))
    log = []
    tr = run_mtt.run(args, log=log)
    steps = _steps(log, 2)
    d = os.path.join(save, "Baseline_MTT", "toy_ipc1_100.0")
    assert sorted(os.listdir(d)) == ["images_0.pt"]
    start = torch.load(os.path.join(d, "images_0.pt"))
    assert tr.image_syn.is_cuda and tuple(start.shape) == (C, T, 3, HW, HW) and not torch.equal(tr.image_syn.cpu(), start)
    assert tr.ops.flat is not None and tr.ops.flat.n == 3641603          # the chain ran on the vdt_ kernels
    assert steps[0]["Synthetic_LR"] == pytest.approx(0.01, rel=1e-6) and steps[1]["Synthetic_LR"] != steps[0]["Synthetic_LR"]


def test_s2d_run_on_the_gpu(files):
    from video_distillation_amd import checkpoint, run_mtt
    save = str(files["dir"] / "s2d")
    args = run_mtt.build_parser("s2d").parse_args(_argv(files, "s2d", save, "--no_eval", "--vpc", "1", "--spc", "2", "--dpc", "2",
                                                       "--path_static", files["static"], "--lr_static", "0.5", "--lr_dynamic=10.0",
                                                       "--lr_hal=1e-4"))
    log = []
    tr = run_mtt.run(args, log=log)
    steps = _steps(log, 2)
    d = os.path.join(save, "S2D_multis_MTT", "toy_ipc1_10.0_0.0001")
    assert sorted(os.listdir(d)) == ["dynamic_0.pt", "hal_0.pt", "images_0.pt"]
    dyn0 = torch.load(os.path.join(d, "dynamic_0.pt"))
    w0 = checkpoint.load_hallucinators(os.path.join(d, "hal_0.pt"))[0][0]
    assert not torch.equal(tr.dynamic.cpu(), dyn0) and not torch.equal(tr.hal_w.cpu().view(-1), w0.view(-1))
    assert not torch.equal(tr.static.cpu(), torch.load(files["static"])["image"])
    assert steps[0]["Synthetic_LR"] == steps[1]["Synthetic_LR"] == pytest.approx(0.01, rel=1e-6)          # no --train_lr
    assert tr.ops.flat.n == 3641603


def test_a_run_with_evaluation_logs_the_accuracy_and_writes_the_best_files(files):
    from video_distillation_amd import run_mtt
    save = str(files["dir"] / "eval")
    args = run_mtt.build_parser("images").parse_args(_argv(files, "images", save, "--num_eval", "1", "--epoch_eval_train", "1",
                                                          "--eval_it", "1", "--Iteration", "0", "--lr_teacher", "0.01"))
    log = []
    run_mtt.run(args, log=log)
    acc = [r for r in log if "Accuracy/ConvNet3D" in r]
    assert [r["step"] for r in acc] == [0]
    assert acc[0]["Accuracy/ConvNet3D"] == pytest.approx(1.0 / 3.0) == acc[0]["Max_Accuracy/ConvNet3D"]
    assert acc[0]["Std/ConvNet3D"] == 0.0
    d = os.path.join(save, "Baseline_MTT", "toy_ipc1_1")
    assert sorted(os.listdir(d)) == ["images_0.pt", "images_best.pt"]
    assert torch.equal(torch.load(os.path.join(d, "images_0.pt")), torch.load(os.path.join(d, "images_best.pt")))
    _steps(log, 1)
