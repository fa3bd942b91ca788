"""``run_frepo`` end to end on the GPU, after the toy-file pattern of tests/test_gpu_mtt_driver.py: both kinds of memories for
two iterations, and one run with evaluation on."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

C, PER, T, HW = 3, 2, 8, 64


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("frepo_gpu")
    g = torch.Generator().manual_seed(8)
    clips = torch.randn(C * PER, T, 3, HW, HW, generator=g)
    # six test clips that are ONE clip under the labels 0 0 1 1 2 2: whatever a network answers, it is right twice in six, so
    # the first evaluation is a new best (accuracy 1/3 > 0) whatever its seed
    test_clips = clips[:1].expand(6, -1, -1, -1, -1).contiguous()
    torch.save({"clips": clips, "labels": torch.arange(C).repeat(PER), "test_clips": test_clips,
                "test_labels": torch.arange(C).repeat_interleave(2)}, d / "toy.pt")
    torch.save({"image": torch.randn(C, 3, HW, HW, generator=g)}, d / "static.pt")
    return {"data": str(d / "toy.pt"), "static": str(d / "static.pt"), "dir": d}


def _argv(files, memories, save, *extra):
    return ["--memories", memories, "--dataset", "toy", "--data_file", files["data"], "--save_path", save, "--im_size", str(HW),
            "--frames", str(T), "--Iteration", "2", "--num_nn_state", "2", "--max_online_updates", "4", "--seed", "4"] + list(extra)


def _steps(log, iterations):
    steps = [r for r in log if "Loss" in r]
    assert [r["step"] for r in steps] == list(range(1, iterations + 1))
    for r in steps:
        assert all(math.isfinite(r[k]) for k in ("Loss", "ln_loss", "lb_loss", "lr"))
        assert r["Loss"] == pytest.approx(r["ln_loss"] + r["lb_loss"], rel=1e-5, abs=1e-6) and r["ln_loss"] > 0
    assert steps[0]["lr"] == pytest.approx(1e-3) and steps[1]["lr"] < steps[0]["lr"]
    return steps


def test_images_run_on_the_gpu(files):
    from video_distillation_amd import run_frepo
    save = str(files["dir"] / "images")
    log = []
    tr = run_frepo.run(run_frepo.build_parser().parse_args(_argv(files, "images", save, "--no_eval", "--init", "real", "--learn_label")), log=log)
    _steps(log, 2)
    d = os.path.join(save, "Baseline_FRePo", "toy_ipc1_100.0_0.001")
    assert sorted(os.listdir(d)) == ["images_1.pt", "y_syn_1.pt"]
    start, y0 = torch.load(os.path.join(d, "images_1.pt")), torch.load(os.path.join(d, "y_syn_1.pt"))
    assert tuple(start.shape) == (C, T, 3, HW, HW) and tuple(y0.shape) == (C, C) and start.dtype == y0.dtype == torch.float32
    blob = torch.load(files["data"])
    assert all(any(torch.equal(start[c], clip) for clip, lab in zip(blob["clips"], blob["labels"]) if int(lab) == c) for c in range(C))
    assert tr.syndata.x_syn.is_cuda and not torch.equal(tr.syndata.x_syn.detach().cpu(), start)
    assert not torch.equal(tr.syndata.y_syn.detach().cpu(), y0)          # --learn_label
    assert len(tr.pools) == 2 and all(0 <= e.step < 4 for e in tr.pools)


def test_s2d_run_on_the_gpu(files):
    from video_distillation_amd import checkpoint, run_frepo, utils
    save = str(files["dir"] / "s2d")
    log = []
    tr = run_frepo.run(run_frepo.build_parser().parse_args(_argv(files, "s2d", save, "--no_eval", "--path_static", files["static"],
                                                                 "--n_hal", "2", "--lr_d=10.0", "--lr_h=1e-4")), log=log)
    steps = [r for r in log if "Loss" in r]
    assert [r["step"] for r in steps] == [1, 2] and all(math.isfinite(r["Loss"]) for r in steps) and steps[0]["lr"] == pytest.approx(1e-4)
    d = os.path.join(save, "S2D_FRePo", "toy_ipc1_10.0_0.0001")
    assert sorted(os.listdir(d)) == ["dynamic_1.pt", "hal_1.pt", "y_syn_1.pt"]
    dyn0, y0 = torch.load(os.path.join(d, "dynamic_1.pt")), torch.load(os.path.join(d, "y_syn_1.pt"))
    assert tuple(dyn0.shape) == (C, 1, T, 1, HW, HW) and tuple(y0.shape) == (C, C)
    hals = checkpoint.load_hallucinators(os.path.join(d, "hal_1.pt"))
    assert len(hals) == 2 and all(tuple(w.shape) == (3, 4, 3, 3, 3) and tuple(b.shape) == (3,) for w, b in hals)
    state = torch.load(os.path.join(d, "hal_1.pt"))
    assert sorted(state) == sorted(torch.nn.ModuleList([utils.Conv3DNet() for _ in range(2)]).state_dict())
    assert not torch.equal(tr.syndata.dynamic.detach().cpu(), dyn0)
    assert torch.equal(tr.syndata.static.detach().cpu(), torch.load(files["static"])["image"])          # the static memory never moves
    assert torch.equal(tr.syndata.y_syn.detach().cpu(), y0)          # no --learn_label
    assert any(not torch.equal(h.encoder.weight.detach().cpu(), w) for h, (w, _) in zip(tr.syndata.hallucinator, hals))


def test_a_run_with_evaluation_logs_the_accuracy_and_writes_the_best_files(files):
    from video_distillation_amd import run_frepo
    save = str(files["dir"] / "eval")
    log = []
    run_frepo.run(run_frepo.build_parser().parse_args(_argv(files, "images", save, "--init", "noise", "--num_eval", "1", "--epoch_eval_train", "1",
                                                            "--eval_it", "1", "--startIt", "1", "--Iteration", "1")), log=log)
    acc = [r for r in log if "Accuracy/ConvNet3D" in r]
    assert [r["step"] for r in acc] == [1]
    assert acc[0]["Accuracy/ConvNet3D"] == pytest.approx(1.0 / 3.0) == acc[0]["Max_Accuracy/ConvNet3D"] and acc[0]["Std/ConvNet3D"] == 0.0
    d = os.path.join(save, "Baseline_FRePo", "toy_ipc1_100.0_0.001")
    assert sorted(os.listdir(d)) == ["images_1.pt", "images_best.pt", "y_syn_1.pt", "y_syn_best.pt"]
    assert torch.equal(torch.load(os.path.join(d, "images_1.pt")), torch.load(os.path.join(d, "images_best.pt")))
    assert [r["step"] for r in log if "Loss" in r] == [1]
