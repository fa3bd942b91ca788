"""``run_s2d`` (the DM branch of distill_s2d_ms.py as a driver) on the CPU with the oracle as compute backend: flags, rejected
settings, three iterations against a hand-driven ``S2DTrainer``, the files it writes, two ranks under gloo against one; and the
host halves of the device-composed multi-static batches (``MultiStaticSharedDataset.draw``, ``hip.hallucinate_multi``'s index
validation).  Toy data: C = 3, 5 clips per class, 64x64x8, vpc 1 / spc 2 / dpc 2."""
import functools
import os
import random

import numpy as np
import pytest
import torch
import torch.distributed as dist

from tests.cpu_backend import OracleBackend
from tests.test_distributed_cpu import _spawn
from video_distillation_amd import checkpoint, distill, hip, run_s2d, utils

C, PER, T, HW = 3, 5, 8, 64
SEED, STATIC_SEED, DATA_SEED = 11, 23, 5
LR_DYNAMIC, LR_HAL = 0.01, 1e-6


def _argv(data_file, save_path, *extra):
    return ["--method", "DM", "--dataset", "toy", "--data_file", data_file, "--save_path", save_path, "--im_size", str(HW),
            "--frames", str(T), "--vpc", "1", "--spc", "2", "--dpc", "2", "--batch_real", "2", "--Iteration", "2", "--eval_it", "2",
            "--n_hal", "2", "--seed", str(SEED), "--lr_dynamic=%s" % LR_DYNAMIC, "--lr_hal=%s" % LR_HAL] + list(extra)


def _toy_clips():
    g = torch.Generator().manual_seed(DATA_SEED)
    return torch.randn(C * PER, T, 3, HW, HW, generator=g), torch.arange(C).repeat_interleave(PER)


def _static():
    return torch.randn(C * 2, 3, HW, HW, generator=torch.Generator().manual_seed(STATIC_SEED))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("s2d")
    clips, labels = _toy_clips()
    perm = torch.arange(C * PER).view(C, PER).t().reshape(-1)          # classes interleaved: the driver's stable sort by class undoes it
    torch.save({"clips": clips[perm], "labels": labels[perm]}, d / "toy.pt")
    torch.save({"image": _static()}, d / "static.pt")
    return {"data": str(d / "toy.pt"), "static": str(d / "static.pt"), "dir": d}


@pytest.fixture(scope="module")
def one_rank(files):
    """Three iterations (0, 1, 2) on one rank, static memory from the file and frozen, no evaluation."""
    save = str(files["dir"] / "one_rank")
    args = run_s2d.build_parser().parse_args(_argv(files["data"], save, "--no_eval", "--no_train_static", "--path_static", files["static"]))
    log = []
    trainer = run_s2d.run(args, backend=OracleBackend(), log=log)
    static, dynamic = trainer.gather_memories()
    return {"log": log, "trainer": trainer, "static": static.clone(), "dynamic": dynamic.clone(),
            "dir": os.path.join(save, "S2D_multis_DM", "toy_ipc1_%s_%s" % (LR_DYNAMIC, LR_HAL))}


def test_parser_accepts_the_flags_of_the_reference_launchers():
    a = run_s2d.build_parser().parse_args(
        ["--method", "DM", "--dataset", "miniUCF101", "--num_eval", "5", "--vpc", "5", "--spc", "10", "--dpc", "10",
         "--epoch_eval_train", "1000", "--lr_dynamic=1e-3", "--lr_hal=1e-5", "--model=ConvNet3D", "--batch_real", "64",
         "--Iteration", "5000", "--eval_mode", "SS", "--eval_it", "500", "--no_train_static", "--path_static", "s.pt",
         "--startIt", "0", "--preload", "--save_path", "out"])
    assert (a.vpc, a.spc, a.dpc, a.lr_dynamic, a.lr_hal, a.no_train_static, a.preload) == (5, 10, 10, 1e-3, 1e-5, True, True)
    d = run_s2d.build_parser().parse_args([])          # the reference's defaults (distill_s2d_ms.py:453-502)
    assert (d.dataset, d.spc, d.dpc, d.vpc, d.eval_mode, d.num_eval, d.eval_it, d.epoch_eval_train, d.Iteration) == \
        ('miniUCF101', 10, 1, 5, 'S', 5, 100, 1000, 15000)
    assert (d.lr_static, d.lr_dynamic, d.lr_teacher, d.lr_hal, d.batch_real, d.batch_train, d.n_hal, d.frames, d.startIt) == \
        (100, 0.01, 0.01, 0.01, 256, 256, 1, 16, 0)
    with pytest.raises(SystemExit):
        run_s2d.build_parser().parse_args(["--method", "MTT"])


def test_settings_the_index_formulas_run_out_of_range_on_are_rejected(files):
    parse = run_s2d.build_parser().parse_args
    with pytest.raises(ValueError, match=r"--dpc 1 with --vpc 5 indexes out of range"):
        run_s2d.run(parse(["--data_file", files["data"], "--vpc", "5", "--dpc", "1"]), backend=OracleBackend())
    with pytest.raises(ValueError, match="out of range"):
        run_s2d.run(parse(["--data_file", files["data"], "--vpc", "2", "--spc", "2", "--dpc", "4", "--no_eval"]), backend=OracleBackend())
    with pytest.raises(ValueError, match="MultiStaticSharedDataset"):
        run_s2d.run(parse(["--data_file", files["data"], "--vpc", "1", "--spc", "4", "--dpc", "2"]), backend=OracleBackend())
    with pytest.raises(ValueError, match="dpc >= 10"):
        run_s2d.run(parse(["--data_file", files["data"], "--vpc", "1", "--spc", "10", "--dpc", "2"]), backend=OracleBackend())


def test_three_iterations_equal_a_hand_driven_trainer(files, one_rank):
    log, tr = one_rank["log"], one_rank["trainer"]
    assert [r["step"] for r in log if "Loss" in r] == [0, 2]          # every 10 iterations and at the end
    assert not any(k.startswith("Accuracy") for r in log for k in r)
    # the same tensors by hand: data sorted by class, dynamic from Generator(seed), hallucinators after manual_seed(seed)
    clips, _ = _toy_clips()
    pool = distill.RealPool(clips, [PER] * C, [PER * c for c in range(C)])
    dynamic = torch.randn(C, 2, T, 1, HW, HW, generator=torch.Generator().manual_seed(SEED))
    torch.manual_seed(SEED)
    hals = [utils.Conv3DNet() for _ in range(2)]
    hand = distill.S2DTrainer(OracleBackend(), pool, C, 1, 2, 2, 2, _static(), dynamic, hals[0].encoder.weight.detach(),
                              hals[0].encoder.bias.detach(), lr_dynamic=LR_DYNAMIC, lr_hal=LR_HAL, lr_static=100.0,
                              train_static=False, momentum=0.95)
    losses = [float(hand.global_loss(hand.step(it, overlap=True))) / C for it in range(3)]
    hand.sync()
    assert [r["Loss"] for r in log if "Loss" in r] == [losses[0], losses[2]]
    assert all(np.isfinite(losses)) and losses[0] != losses[2]
    assert torch.equal(tr.dynamic, hand.dynamic) and torch.equal(tr.hal_w, hand.hal_w) and torch.equal(tr.hal_b, hand.hal_b)
    start = torch.randn(C, 2, T, 1, HW, HW, generator=torch.Generator().manual_seed(SEED))          # (`dynamic` is the shard's storage)
    assert not torch.equal(tr.dynamic, start.view(-1, T, 1, HW, HW))          # it was trained
    # the static memory of the file is what the trainer holds (frozen: still those bits after the steps)
    assert torch.equal(tr.static, _static()) and tr.buf_s is None


def test_files_written_at_iteration_zero(files, one_rank):
    d = one_rank["dir"]
    dyn0 = torch.load(os.path.join(d, "dynamic_0.pt"))
    assert tuple(dyn0.shape) == (C * 2, T, 1, HW, HW)
    assert torch.equal(dyn0, torch.randn(C, 2, T, 1, HW, HW, generator=torch.Generator().manual_seed(SEED)).view(-1, T, 1, HW, HW))
    pairs = checkpoint.load_hallucinators(os.path.join(d, "hal_0.pt"))
    assert len(pairs) == 2 and all(tuple(w.shape) == (3, 4, 3, 3, 3) and tuple(b.shape) == (3,) for w, b in pairs)
    assert not torch.equal(pairs[0][0], pairs[1][0])
    # iteration 2 is an evaluation iteration too, but without a new best accuracy only multiples of 1000 are saved
    assert sorted(os.listdir(d)) == ["dynamic_0.pt", "hal_0.pt"]          # --no_train_static: no images_*.pt


def test_a_trained_static_memory_is_saved_as_images(files):
    save = str(files["dir"] / "train_static")
    args = run_s2d.build_parser().parse_args(_argv(files["data"], save, "--no_eval", "--path_static", files["static"],
                                                   "--Iteration", "0", "--lr_static", "0.5"))
    tr = run_s2d.run(args, backend=OracleBackend(), log=[])
    d = os.path.join(save, "S2D_multis_DM", "toy_ipc1_%s_%s" % (LR_DYNAMIC, LR_HAL))
    assert sorted(os.listdir(d)) == ["dynamic_0.pt", "hal_0.pt", "images_0.pt"]
    assert torch.equal(torch.load(os.path.join(d, "images_0.pt")), _static())          # saved before the step of iteration 0
    assert tr.train_static and not torch.equal(tr.static, _static())


def _worker_two_ranks(rank, world, port, q, data, static, save):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank); os.environ["WORLD_SIZE"] = str(world); os.environ["LOCAL_RANK"] = "0"
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        args = run_s2d.build_parser().parse_args(_argv(data, save, "--no_eval", "--no_train_static", "--path_static", static))
        log = []
        tr = run_s2d.run(args, backend=OracleBackend(), log=log)
        st, dy = tr.gather_memories()          # (a collective: both ranks)
        if rank == 0:
            q.put(([(r["step"], r["Loss"]) for r in log if "Loss" in r], st.numpy(), dy.numpy(), tr.hal_w.numpy(), tr.hal_b.numpy(),
                   tuple(tr.dynamic.shape)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_gloo_match_one_rank(files, one_rank):
    save = str(files["dir"] / "two_ranks")
    losses, st, dy, hal_w, hal_b, shard = _spawn(functools.partial(_worker_two_ranks, data=files["data"], static=files["static"],
                                                                   save=save), 2)
    want = [(r["step"], r["Loss"]) for r in one_rank["log"] if "Loss" in r]
    assert [s for s, _ in losses] == [s for s, _ in want]
    for (_, got), (_, ref) in zip(losses, want):
        assert abs(got / ref - 1) < 1e-5
    tr = one_rank["trainer"]
    np.testing.assert_allclose(hal_w, tr.hal_w.numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(hal_b, tr.hal_b.numpy(), rtol=1e-5, atol=1e-7)
    assert shard == (2 * 2, T, 1, HW, HW)          # rank 0 owns classes 0 and 1 of 3 ...
    assert dy.shape == (C, 2, T, 1, HW, HW) and st.shape == (C * 2, 3, HW, HW)          # ... and gathers all three, in class order
    np.testing.assert_allclose(dy, one_rank["dynamic"].numpy(), rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(st, one_rank["static"].numpy())
    assert os.path.exists(os.path.join(save, "S2D_multis_DM", "toy_ipc1_%s_%s" % (LR_DYNAMIC, LR_HAL), "dynamic_0.pt"))


def test_gather_memories_on_one_rank_returns_views_of_the_shards(one_rank):
    tr = one_rank["trainer"]
    st, dy = tr.gather_memories()
    assert st.data_ptr() == tr.static.data_ptr() and dy.data_ptr() == tr.dynamic.data_ptr()
    assert tuple(dy.shape) == (C, 2, T, 1, HW, HW) and tuple(st.shape) == (C * 2, 3, HW, HW)


@pytest.mark.parametrize("n_c,per_s,dpc", [(3, 2, 2), (2, 10, 10)])
def test_draw_consumes_random_as_getitem_does(n_c, per_s, dpc):
    # memories whose values name their row, hallucinators that name themselves: an item tells what it was composed from
    static = torch.arange(n_c * per_s, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 3, 2, 2)
    dynamic = torch.arange(n_c * dpc, dtype=torch.float32).view(n_c, dpc, 1, 1, 1, 1).expand(-1, -1, 2, 1, 2, 2)
    hals = [lambda s, d, k=k: torch.stack([s[:, 0, 0, 0], d[:, 0, 0, 0, 0], torch.full((1,), float(k))], 1) for k in range(3)]
    ds = utils.MultiStaticSharedDataset(static, dynamic, hals)
    assert len(ds) == (n_c if per_s == 2 else n_c * 5)
    items = list(range(len(ds))) * 3
    random.seed(99)
    got = [ds[i] for i in items]
    after_items = random.getstate()
    random.seed(99)
    draws = [ds.draw(i) for i in items]
    assert random.getstate() == after_items
    for (video, label), (lab, si, di, hi) in zip(got, draws):
        assert label == lab and video.tolist() == [float(si), float(lab * dpc + di), float(hi)]
        assert lab * per_s <= si < (lab + 1) * per_s and 0 <= di < dpc and 0 <= hi < 3
    assert len({d[1:] for d in draws}) > len(ds) // 2          # (the draws are drawn, not constant)


def test_hallucinate_multi_validates_its_tables_before_any_device_call(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hip, "lib", no_device)
    static, dynamic = torch.zeros(4, 3, 6, 10), torch.zeros(5, 2, 1, 6, 10)
    w, b = torch.zeros(2, 3, 4, 3, 3, 3), torch.zeros(2, 3)
    for sidx, didx, hidx, what in (([0, 4], [0, 1], [0, 1], "sidx 4"), ([0, -1], [0, 1], [0, 1], "sidx -1"),
                                   ([0, 1], [5, 1], [0, 1], "didx 5"), ([0, 1], [0, 1], [0, 2], "hidx 2"),
                                   ([0, 1], [0, 1], [-1, 0], "hidx -1")):
        with pytest.raises(ValueError, match=what):
            hip.hallucinate_multi(static, dynamic, sidx, didx, hidx, w, b)
    with pytest.raises(ValueError, match="indices"):
        hip.hallucinate_multi(static, dynamic, [0, 1], [0], [0, 1], w, b)
    for extra in ([1], [1, 2, 0]):          # what rides along has one entry per clip, or the packed layout shifts
        with pytest.raises(ValueError, match="extra holds %d entries for 2 clips" % len(extra)):
            hip.hallucinate_multi(static, dynamic, [3, 0], [4, 0], [1, 0], w, b, extra=extra)
    with pytest.raises(RuntimeError, match="no CPU path"):          # tables in range: only then are the tensors looked at
        hip.hallucinate_multi(static, dynamic, [3, 0], [4, 0], [1, 0], w, b)
    assert not utils.MultiStaticBatches.device_composable(static, torch.zeros(2, 2, 2, 1, 6, 10), [utils.Conv3DNet()])
