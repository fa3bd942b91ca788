"""The evaluation rounds of ``run_dm``, ``run_s2d`` and ``run_mtt`` (both kinds of memories) on the CPU with the oracle as compute
backend.  ``ConvNet3D`` has no CPU path, so ``utils.get_network``, ``utils.evaluate_synset`` and ``evalpool.evaluate_pool`` are
replaced by stubs that record what they are given and return scripted accuracies; everything around them -- which of the two is
called with what, the log records, the ``best_*`` bookkeeping, the files -- is the drivers' own code and is pinned here.

Toy data: C = 3, 8 frames, 64x64, a ``--data_file`` with ``test_clips``; ``--num_eval 2 --Iteration 2 --eval_it 1``: three
evaluations whose scripted accuracies rise (0.375, 0.625: a new best each) and then fall (0.1875: not a new best)."""
import json
import os

import pytest
import torch

from tests.cpu_backend import OracleBackend, OracleMTTOps
from tests.test_traj_cpu import _random_walk
from video_distillation_amd import checkpoint, evalpool, run_dm, run_mtt, run_s2d, utils

C, PER, T, HW, IPC = 3, 5, 8, 64, 2
NUM_EVAL, EVAL_SEED, SEED = 2, 7, 4
ACCS = [[0.25, 0.5], [0.5, 0.75], [0.125, 0.25]]          # per evaluation, per network: binary fractions, so mean and std are exact
MEAN_STD = [(0.375, 0.125), (0.625, 0.125), (0.1875, 0.0625)]
BEST = [(0.375, 0.125), (0.625, 0.125), (0.625, 0.125)]          # Max_Accuracy / Max_Std after each evaluation
TIMES = {"train_s": [0.5, 0.25], "test_pass_s": [[0.125] * 3] * 2}
REFUSAL = r"--eval_ranks all evaluates ConvNet3D \(the hot path's network\), not ConvNet3DBN"
LABELS = [c for c in range(C) for _ in range(IPC)]
DRIVERS = ["dm", "s2d", "mtt_images", "mtt_s2d"]
MODE = {"dm": "none", "s2d": "multi-static", "mtt_images": "none", "mtt_s2d": "multi-static"}
SAVE_DIR = {"dm": "Baseline_DM/toy_ipc2_0.1", "s2d": "S2D_multis_DM/toy_ipc1_0.01_0.0001",
            "mtt_images": "Baseline_MTT/toy_ipc2_100.0", "mtt_s2d": "S2D_multis_MTT/toy_ipc1_10.0_0.0001"}
BEST_NAME = {"images_%s.pt": "images_best.pt", "dynamic_%s.pt": "dynamic_best.pt", "hal_%s.pt": "weights_best.pt"}
NUMBERED = {"dm": ["images_%s.pt"], "mtt_images": ["images_%s.pt"]}
NUMBERED["s2d"] = NUMBERED["mtt_s2d"] = ["dynamic_%s.pt", "hal_%s.pt", "images_%s.pt"]          # (the static memory is trained: images_*)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("driver_eval")
    g = torch.Generator().manual_seed(3)
    clips = torch.randn(C * PER, T, 3, HW, HW, generator=g)
    labels = torch.arange(C).repeat(PER)          # classes interleaved
    torch.save({"clips": clips, "labels": labels, "test_clips": clips[:4], "test_labels": labels[:4]}, d / "toy.pt")
    torch.save({"clips": clips, "labels": labels}, d / "no_test.pt")
    torch.save({"image": torch.randn(C * 2, 3, HW, HW, generator=g)}, d / "static.pt")
    checkpoint.save_expert_buffer(str(d / "buffers"), _random_walk(g, 2, 3))
    return {"data": str(d / "toy.pt"), "no_test": str(d / "no_test.pt"), "static": str(d / "static.pt"),
            "buffers": str(d / "buffers"), "dir": d}


def _run(files, driver, save, *extra, data="data"):
    """One run of `driver` with the toy settings -> (trainer, log)."""
    common = ["--dataset", "toy", "--data_file", files[data], "--save_path", save, "--im_size", str(HW), "--frames", str(T),
              "--num_eval", str(NUM_EVAL), "--Iteration", "2", "--eval_it", "1", "--batch_train", "32"]
    s2d = ["--vpc", "1", "--spc", "2", "--dpc", "2", "--n_hal", "2", "--path_static", files["static"], "--lr_static", "0.5", "--seed", str(SEED)]
    mtt = ["--buffer_path", files["buffers"], "--syn_steps", "2", "--expert_epochs", "1", "--max_start_epoch", "2", "--seed", str(SEED),
           "--lr_teacher", "0.01", "--train_lr", "--lr_lr", "1e-8"]
    log = []
    if driver == "dm":
        argv = common + ["--ipc", str(IPC), "--batch_real", "3", "--lr_img", "0.1", "--lr_net", "0.02", "--epoch_eval_train", "300"]
        return run_dm.run(run_dm.build_parser().parse_args(argv + list(extra)), backend=OracleBackend(), log=log), log
    if driver == "s2d":
        argv = common + s2d + ["--batch_real", "2", "--lr_dynamic=0.01", "--lr_hal=1e-4", "--lr_teacher", "0.03", "--epoch_eval_train", "300"]
        return run_s2d.run(run_s2d.build_parser().parse_args(argv + list(extra)), backend=OracleBackend(), log=log), log
    if driver == "mtt_images":
        argv = ["--memories", "images"] + common + mtt + ["--ipc", str(IPC), "--lr_img", "100", "--epoch_eval_train", "200"]
        return run_mtt.run(run_mtt.build_parser("images").parse_args(argv + list(extra)), ops=OracleMTTOps(), log=log), log
    argv = ["--memories", "s2d"] + common + mtt + s2d + ["--lr_dynamic=10.0", "--lr_hal=1e-4", "--epoch_eval_train", "300"]
    return run_mtt.run(run_mtt.build_parser("s2d").parse_args(argv + list(extra)), ops=OracleMTTOps(), log=log), log


class Spy:
    """Stands in for the three functions the drivers evaluate with; keeps every tensor it was given alive (so that distinct
    ``data_ptr`` means distinct storage) and then overwrites it, as training on it in place would: a driver that handed out its
    trainer's own tensor would log other losses than the run without evaluation."""

    def __init__(self, monkeypatch):
        self.networks, self.synset, self.pool, self.keep = [], [], [], []
        monkeypatch.setattr(utils, "get_network", self.get_network)
        monkeypatch.setattr(utils, "evaluate_synset", self.evaluate_synset)
        monkeypatch.setattr(evalpool, "evaluate_pool", self.evaluate_pool)

    def _memories(self, images, mode):
        tensors = [images] if mode == 'none' else list(images[:2])
        rec = {"ptr": [t.data_ptr() for t in tensors], "shape": [tuple(t.shape) for t in tensors]}
        if mode != 'none':
            assert isinstance(images, list) and len(images) == 3
            rec["n_hal"] = len(images[2])
        self.keep += tensors
        for t in tensors:
            t.fill_(1e3)
        return rec

    def get_network(self, model, channel, num_classes, im_size=(32, 32), frames=16, dist=True):
        self.networks.append((model, channel, num_classes, tuple(im_size), frames, dist))
        return torch.nn.Identity()

    def evaluate_synset(self, it_eval, net, images_train, labels_train, testloader, args, mode='hallucinator', return_loss=False,
                        test_freq=None):
        n = len(self.synset)
        rec = {"it_eval": it_eval, "mode": mode, "test_freq": test_freq, "args": dict(vars(args)), "test_items": len(testloader.dataset),
               "batch_size": testloader.batch_size, "labels": None if labels_train is None else labels_train.tolist()}
        rec.update(self._memories(images_train, mode))
        self.synset.append(rec)
        return net, 1.0, ACCS[n // NUM_EVAL][n % NUM_EVAL], None

    def evaluate_pool(self, make_net, images_train, labels_train, testloader, args, *, num_eval, seed, mode='none', rank=0, world=1,
                      num_classes=None, on_trained=None):
        n = len(self.pool)
        assert callable(make_net) and on_trained is None
        rec = {"num_eval": num_eval, "seed": seed, "mode": mode, "rank": rank, "world": world, "num_classes": num_classes,
               "args": dict(vars(args)), "test_items": len(testloader.dataset),
               "labels": None if labels_train is None else labels_train.tolist()}
        rec.update(self._memories(images_train, mode))
        self.pool.append(rec)
        return {"mean": MEAN_STD[n][0], "std": MEAN_STD[n][1], "times": TIMES, "assignment": evalpool.assignment(num_eval, world)}


def _lines(log):
    """The log as the JSON lines written, without the clock."""
    return [json.dumps({k: v for k, v in r.items() if k != "elapsed_s"}) for r in log]


def _accuracy(it):
    (mean, std), (best, best_std) = MEAN_STD[it], BEST[it]
    return json.dumps({"step": it, "Accuracy/ConvNet3D": mean, "Max_Accuracy/ConvNet3D": best, "Std/ConvNet3D": std,
                       "Max_Std/ConvNet3D": best_std})


def _tree(save):
    return sorted(os.path.relpath(os.path.join(d, f), save) for d, _, fs in os.walk(save) for f in fs)


def _files_of(driver, its, best):
    return sorted("%s/%s" % (SAVE_DIR[driver], f % it) for f in NUMBERED[driver] for it in its) + \
        (sorted("%s/%s" % (SAVE_DIR[driver], BEST_NAME[f]) for f in NUMBERED[driver]) if best else [])


@pytest.fixture(scope="module")
def no_eval(files):
    """Every driver once with ``--no_eval``: the training records the runs with evaluation must repeat, and the files."""
    out = {}
    for driver in DRIVERS:
        save = str(files["dir"] / ("no_eval_" + driver))
        tr, log = _run(files, driver, save, "--no_eval")
        out[driver] = {"trainer": tr, "lines": _lines(log), "tree": _tree(save)}
    return out


def _expected_lines(driver, train, after_accuracy=lambda it: []):
    """The records of a run with evaluation: `train` are those of the run without, `after_accuracy(it)` what follows an accuracy
    record.  DM logs the loss at iterations 0 and 2; MTT has a header first and writes iteration 1's loss out before it
    evaluates at iteration 2."""
    acc = [[_accuracy(it)] + after_accuracy(it) for it in range(3)]
    if driver in ("dm", "s2d"):
        loss0, loss2 = train
        return acc[0] + [loss0] + acc[1] + acc[2] + [loss2]
    header, g0, g1, g2 = train
    return [header] + acc[0] + [g0] + acc[1] + [g1] + acc[2] + [g2]


def _check_trained_alike(driver, tr, ref):
    for name in (("image_syn",) if MODE[driver] == 'none' else ("static", "dynamic", "hal_w", "hal_b")):
        assert torch.equal(getattr(tr, name), getattr(ref, name)), name


def _check_files(driver, save):
    # a new best at iterations 0 and 1, none at 2: the checkpoint calls write the numbered files of every iteration they save
    # at, so 0 (a multiple of 1000 too) and 1 have them and 2 has none; *_best hold iteration 1
    assert _tree(save) == sorted(_files_of(driver, (0, 1), best=True))
    d = os.path.join(save, SAVE_DIR[driver])
    for numbered in NUMBERED[driver]:
        a, b = torch.load(os.path.join(d, numbered % 1)), torch.load(os.path.join(d, BEST_NAME[numbered]))
        if isinstance(a, dict):
            assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
        else:
            assert torch.equal(a, b) and float(a.abs().max()) < 1e3          # (not what the stubs wrote over their copies)
        assert not _same(torch.load(os.path.join(d, numbered % 0)), a), numbered          # iteration 1's, not iteration 0's


def _same(a, b):
    return all(torch.equal(a[k], b[k]) for k in a) if isinstance(a, dict) else torch.equal(a, b)


def _eargs(driver, lr_net):
    return {"device": "cpu", "lr_net": lr_net, "epoch_eval_train": 200 if driver == "mtt_images" else 300, "batch_train": 32,
            "model": "ConvNet3D", "eval_mode": "SS" if driver == "dm" else "S"}


def _lr_net(driver, lines, it):
    """--lr_net for DM, --lr_teacher for run_s2d, for MTT the syn_lr the step of iteration `it` started from."""
    if driver in ("dm", "s2d"):
        return {"dm": 0.02, "s2d": 0.03}[driver]
    return [r for r in map(json.loads, lines) if r.get("step") == it and "Synthetic_LR" in r][0]["Synthetic_LR"]


def _check_memories(driver, rec, trainer):
    if MODE[driver] == 'none':
        assert rec["shape"] == [(C * IPC, T, 3, HW, HW)] and rec["labels"] == LABELS
        live = [trainer.image_syn]
    else:
        assert rec["shape"] == [(C * 2, 3, HW, HW), (C, 2, T, 1, HW, HW)] and rec["n_hal"] == 2 and rec["labels"] is None
        live = [trainer.static, trainer.dynamic]
    assert not set(rec["ptr"]) & {t.data_ptr() for t in live}


@pytest.mark.parametrize("driver", DRIVERS)
def test_rank0_evaluation_round(driver, files, no_eval, monkeypatch):
    spy = Spy(monkeypatch)
    save = str(files["dir"] / ("rank0_" + driver))
    tr, log = _run(files, driver, save)
    lines = _lines(log)
    assert lines == _expected_lines(driver, no_eval[driver]["lines"])
    _check_trained_alike(driver, tr, no_eval[driver]["trainer"])
    _check_files(driver, save)
    assert spy.pool == []
    assert spy.networks == [("ConvNet3D", 3, C, (HW, HW), T, False)] * (3 * NUM_EVAL)
    assert len(spy.synset) == 3 * NUM_EVAL
    if driver.startswith("mtt"):          # --train_lr: every evaluation sees another syn_lr
        assert len({_lr_net(driver, lines, it) for it in range(3)}) == 3
    for n, rec in enumerate(spy.synset):
        it = n // NUM_EVAL
        assert rec["it_eval"] == n % NUM_EVAL and rec["mode"] == MODE[driver]
        assert rec["test_freq"] == (200 if driver == "mtt_images" else None)
        assert rec["args"] == _eargs(driver, _lr_net(driver, lines, it))
        assert rec["test_items"] == 4 and rec["batch_size"] == 64
        _check_memories(driver, rec, tr)
    if MODE[driver] == 'none':          # every network trains on a copy of its own
        assert len({rec["ptr"][0] for rec in spy.synset}) == 3 * NUM_EVAL


@pytest.mark.parametrize("driver", DRIVERS)
def test_eval_ranks_all_evaluation_round(driver, files, no_eval, monkeypatch):
    spy = Spy(monkeypatch)
    save = str(files["dir"] / ("all_" + driver))
    tr, log = _run(files, driver, save, "--eval_ranks", "all", "--eval_seed", str(EVAL_SEED))
    lines = _lines(log)
    seed_record = json.dumps({"eval_ranks": "all", "eval_seed": EVAL_SEED, "world": 1})
    timing = lambda it: [json.dumps({"step": it, "eval_pool": {"train_s": TIMES["train_s"], "test_pass_s": TIMES["test_pass_s"],
                                                               "assignment": evalpool.assignment(NUM_EVAL, 1)}})]
    want = _expected_lines(driver, no_eval[driver]["lines"], timing if driver == "dm" else (lambda it: []))
    assert lines == [seed_record] + want          # (the seed record is the first of all, before MTT's header)
    _check_trained_alike(driver, tr, no_eval[driver]["trainer"])
    _check_files(driver, save)
    assert spy.synset == [] and spy.networks == [] and len(spy.pool) == 3
    for it, rec in enumerate(spy.pool):
        assert (rec["seed"], rec["mode"], rec["num_eval"], rec["rank"], rec["world"], rec["num_classes"]) == \
            (EVAL_SEED + it, MODE[driver], NUM_EVAL, 0, 1, C)
        assert rec["args"] == _eargs(driver, _lr_net(driver, lines, it)) and rec["test_items"] == 4
        _check_memories(driver, rec, tr)


def test_mtt_images_tests_at_the_end_below_200_epochs(files, monkeypatch):
    spy = Spy(monkeypatch)
    _run(files, "mtt_images", str(files["dir"] / "below_200"), "--epoch_eval_train", "199", "--Iteration", "0")
    assert [rec["test_freq"] for rec in spy.synset] == [None] * NUM_EVAL and spy.synset[0]["args"]["epoch_eval_train"] == 199


@pytest.mark.parametrize("driver", DRIVERS)
def test_no_eval_save_cadence(driver, no_eval):
    # run_dm saves inside its evaluation gate; the other two save at multiples of 1000 whether they evaluate or not
    assert no_eval[driver]["tree"] == ([] if driver == "dm" else _files_of(driver, (0,), best=False))
    assert not any("Accuracy" in line or "eval_ranks" in line for line in no_eval[driver]["lines"])


def test_a_clock_seed_is_logged_and_used(files, monkeypatch):
    spy = Spy(monkeypatch)
    _, log = _run(files, "s2d", str(files["dir"] / "clock"), "--eval_ranks", "all", "--Iteration", "0")
    assert sorted(log[0]) == ["eval_ranks", "eval_seed", "world"] and log[0]["eval_ranks"] == "all" and log[0]["world"] == 1
    assert isinstance(log[0]["eval_seed"], int) and 0 <= log[0]["eval_seed"] < 100000
    assert [rec["seed"] for rec in spy.pool] == [log[0]["eval_seed"]]


def test_run_dm_writes_the_seed_record_without_test_clips(tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    argv = ["--dataset", "synthetic", "--num_classes", str(C), "--pool_per_class", "2", "--im_size", str(HW), "--frames", str(T),
            "--batch_real", "2", "--save_path", str(tmp_path), "--Iteration", "0"]
    log = []
    run_dm.run(run_dm.build_parser().parse_args(argv + ["--eval_ranks", "all", "--eval_seed", str(EVAL_SEED)]), backend=OracleBackend(), log=log)
    assert [sorted(r) for r in log] == [["eval_ranks", "eval_seed", "world"], ["Loss", "elapsed_s", "step"]]
    assert log[0] == {"eval_ranks": "all", "eval_seed": EVAL_SEED, "world": 1}
    assert spy.pool == [] and spy.synset == []
    # ... and saves at iteration 0 (its gate is --no_eval alone), which it does not under --no_eval
    assert _tree(str(tmp_path)) == ["Baseline_DM/synthetic_ipc1_1.0/images_0.pt"]
    log = []
    run_dm.run(run_dm.build_parser().parse_args(argv + ["--eval_ranks", "all", "--eval_seed", str(EVAL_SEED), "--no_eval"]),
               backend=OracleBackend(), log=log)
    assert [sorted(r) for r in log] == [["Loss", "elapsed_s", "step"]]


@pytest.mark.parametrize("driver", ["s2d", "mtt_images", "mtt_s2d"])
def test_no_seed_record_where_nothing_is_evaluated(driver, files, monkeypatch):
    spy = Spy(monkeypatch)
    save = str(files["dir"] / ("no_test_" + driver))
    _, log = _run(files, driver, save, "--eval_ranks", "all", "--eval_seed", str(EVAL_SEED), "--Iteration", "0", data="no_test")
    assert not any("eval_ranks" in r or any(k.startswith("Accuracy") for k in r) for r in log)
    assert spy.pool == [] and spy.synset == []
    assert _tree(save) == _files_of(driver, (0,), best=False)


# ---- run_dm's three --memories modes side by side ---------------------------------------------------------------------------
# 2 classes, 8 frames, 64x64, --Iteration 1 --eval_it 1 (evaluation iterations 0 and 1), --eval_ranks all --eval_seed 7, with
# --no_eval and without it on data that has no test split.  The literals were recorded by running the commit BEFORE the three
# modes shared one loop; they differ between the modes on purpose (run_dm's docstring): images and key frames write nothing under
# --no_eval and log the seed whenever they may evaluate; static writes static_0.pt either way and logs no seed without test images.
SEED_KEYS, LOSS_KEYS = ["eval_ranks", "eval_seed", "world"], ["Loss", "elapsed_s", "step"]
THREE_MODES = {
    ("images", "no_eval"): ([], [LOSS_KEYS, LOSS_KEYS]),
    ("images", "no_test"): (["Baseline_DM/synthetic_ipc2_0.1/images_0.pt"], [SEED_KEYS, LOSS_KEYS, LOSS_KEYS]),
    ("static", "no_eval"): (["Static_DM/synthetic_spc2_0.1/static_0.pt"], [LOSS_KEYS, LOSS_KEYS]),
    ("static", "no_test"): (["Static_DM/synthetic_spc2_0.1/static_0.pt"], [LOSS_KEYS, LOSS_KEYS]),
    ("keyframes", "no_eval"): ([], [LOSS_KEYS, LOSS_KEYS]),
    ("keyframes", "no_test"): (["Keyframes_DM/synthetic_ipc2_k3_linear_0.1/keyframes_0.pt"], [SEED_KEYS, LOSS_KEYS, LOSS_KEYS]),
}


def _three_modes_run(memories, flavour, d):
    """-> (files under --save_path, key sets of the log records in order, steps of the records that have one)."""
    argv = ["--memories", memories, "--dataset", "synthetic", "--num_classes", "2", "--pool_per_class", "3", "--ipc", "2", "--spc", "2",
            "--key_frames", "3", "--Iteration", "1", "--eval_it", "1", "--batch_real", "2", "--frames", str(T), "--im_size", str(HW),
            "--lr_img", "0.1", "--num_eval", "1", "--save_path", str(d / "save"), "--eval_ranks", "all", "--eval_seed", "7"]
    if memories == "static":          # (synthetic stills come with test images: a file of stills without any instead)
        g = torch.Generator().manual_seed(5)
        torch.save({"images": torch.randn(6, 3, HW, HW, generator=g), "labels": torch.arange(2).repeat(3)}, d / "stills.pt")
        argv += ["--data_file", str(d / "stills.pt")]
    log = []
    run_dm.run(run_dm.build_parser().parse_args(argv + (["--no_eval"] if flavour == "no_eval" else [])), backend=OracleBackend(), log=log)
    return _tree(str(d / "save")), [sorted(r) for r in log], [r["step"] for r in log if "step" in r]


@pytest.mark.parametrize("memories,flavour", sorted(THREE_MODES))
def test_run_dm_three_modes_files_and_records(memories, flavour, tmp_path, monkeypatch):
    spy = Spy(monkeypatch)
    files_want, keys_want = THREE_MODES[(memories, flavour)]
    tree, keys, steps = _three_modes_run(memories, flavour, tmp_path)
    assert tree == files_want
    assert keys == keys_want and steps == [0, 1]
    assert spy.pool == [] and spy.synset == [] and spy.networks == []          # nothing to evaluate with in either flavour


@pytest.mark.parametrize("driver", DRIVERS)
def test_eval_ranks_all_refuses_other_networks(driver, files, monkeypatch):
    spy = Spy(monkeypatch)
    save = str(files["dir"] / ("refused_" + driver))
    with pytest.raises(NotImplementedError, match=REFUSAL):
        _run(files, driver, save, "--eval_ranks", "all", "--eval_seed", str(EVAL_SEED), "--model", "ConvNet3DBN", "--eval_mode", "SS")
    assert spy.pool == [] and not os.path.exists(save)
