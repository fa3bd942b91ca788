"""run_frepo's device-resident real batches and its leader / embedder protocol on a one-GPU box: ranks share device 0 over gloo
(tests/frepo_ranks_gpu_tool.py, one child per rank, every child under a timeout) in the ordered mode (VD_DETERMINISTIC=1).

What the exchange rests on comes first: ``embed_exact`` treats every clip on its own, so the rows a rank embeds are the rows of
the whole batch's forward, bit for bit.  Then three ranks against one rank -- rank 0 runs the one-rank code on identical
``feat_tar``, so losses, synthetic parameters and pool weights are bit-equal --, a failure on one rank that ends all three, and
``run_frepo`` at two ranks with the evaluation dealt."""
import json
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "frepo_ranks_gpu_tool.py")
UCF = os.path.join(ROOT, "tests", "golden", "frames", "UCF101")
C, PER, T, HW = 3, 2, 8, 64


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _ranks(world, args, timeout=240, check=True):
    """One child per rank, started together; -> [(returncode, stderr)] in rank order.  A child that outlives ``timeout`` is
    killed and fails the test: no rank may be left waiting in a collective."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VD_DETERMINISTIC="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=_free_port(),
               WORLD_SIZE=str(world))
    env.pop("LOCAL_RANK", None)
    procs = [subprocess.Popen([sys.executable, TOOL] + args, cwd=ROOT, env=dict(env, RANK=str(r)), stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(world)]
    out = []
    try:
        with ThreadPoolExecutor(max_workers=world) as ex:
            for p, (_, err) in zip(procs, ex.map(lambda p: p.communicate(timeout=timeout), procs)):
                out.append((p.returncode, err))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    if check:
        for r, (code, err) in enumerate(out):
            assert code == 0, "rank %d of %d: %s" % (r, world, err[-3000:])
    return out


def test_embed_exact_treats_every_clip_on_its_own():
    """``embed_exact(x)[a:b]`` is ``embed_exact(x[a:b])`` bit for bit for the three uneven slices of 8 clips (2 / 3 / 3): a rank's
    rows of the gathered features are the rows of the one-rank forward."""
    from video_distillation_amd import evalpool, frepo
    evalpool.seed_all(5)
    net = evalpool.convnet3d_factory(C, (HW, HW), T)(0).cuda()
    net.eval()
    x = torch.randn(8, T, 3, HW, HW, generator=torch.Generator().manual_seed(6)).cuda()
    whole = net.embed_exact(x).clone()
    assert whole.shape[0] == 8 and whole.dtype == torch.float32 and whole.dim() == 2
    cuts = [frepo.rank_slice(8, r, 3) for r in range(3)]
    assert cuts == [(0, 2), (2, 5), (5, 8)]
    for lo, hi in cuts + [(7, 8)]:
        part = net.embed_exact(x[lo:hi].contiguous())
        assert torch.equal(part.view(torch.int32), whole[lo:hi].view(torch.int32)), (lo, hi)


@pytest.mark.parametrize("memories", ["images", "s2d"])
def test_three_ranks_are_bit_equal_to_one_rank(tmp_path, memories):
    """Three iterations with batches of 8, 3 and 2 clips (slices 2/3/3, 1/1/1 and 0/1/1) at world 3 against ``step(x, y)`` at world
    1: the pool indices, the three losses per step, the synthetic parameters and both pool elements' weights on rank 0, bit for
    bit; every rank ends with rank 0's pool weights.

    With s2d memories this also rests on the ordered form of ``vd_hallucinator_bwd`` (tests/test_gpu_hal_ordered.py): its default
    forms add the hallucinators' weight-gradient partial sums with fp32 atomics in whatever order the workgroups finish, and two
    identical ONE-rank runs then differ in the synthetic parameters by the third step (Adam's first steps hide the last-bit
    differences of the gradient, its moments keep them)."""
    one, three = str(tmp_path / "one"), str(tmp_path / "three")
    with ThreadPoolExecutor(max_workers=2) as ex:          # four children on the card: one one-rank and one three-rank job
        jobs = [ex.submit(_ranks, 1, ["trainer", "--memories", memories, "--out", one]),
                ex.submit(_ranks, 3, ["trainer", "--memories", memories, "--out", three])]
        for j in jobs:
            j.result()
    want = json.load(open(one + ".rank0.json"))
    got = [json.load(open("%s.rank%d.json" % (three, r))) for r in range(3)]
    assert want["finite"] and len(want["losses"]) == 3 and len(set(map(tuple, want["losses"]))) == 3
    for r in (1, 2):          # after the run every rank holds rank 0's pool weights
        assert got[r]["steps"] == 3 and got[r]["weights"] == got[0]["weights"], r
    assert got[0]["picked"] == want["picked"]
    assert got[0]["losses"] == want["losses"], "the three losses per step differ from the one-rank run"
    assert want["weights"][0] != want["weights"][1]
    assert got[0]["syn"] == want["syn"], "the synthetic parameters differ from the one-rank run"
    assert got[0]["weights"] == want["weights"], "the pool weights differ from the one-rank run"


def test_a_rank_that_raises_ends_all_three(tmp_path):
    """Rank 1 raises on the host in its second embed: it carries the flag into the exchange that follows, every rank raises and
    exits non-zero by itself, within the timeout."""
    out = _ranks(3, ["trainer", "--out", str(tmp_path / "fail"), "--fail_rank", "1"], timeout=180, check=False)
    assert all(code not in (0, None) and code > 0 for code, _ in out), [code for code, _ in out]
    assert "injected on rank 1" in out[1][1]
    assert "another rank failed" in out[0][1] and "another rank failed" in out[2][1]
    assert not any(os.path.exists(str(tmp_path / ("fail.rank%d.json" % r))) for r in range(3))


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """A toy data file after tests/test_gpu_frepo_driver.py's, with seven test clips of their own (a short last batch is none
    here: the file loader reads 64 at a time), so that the accuracy depends on the networks."""
    d = tmp_path_factory.mktemp("frepo_ranks")
    g = torch.Generator().manual_seed(8)
    clips = torch.randn(C * PER, T, 3, HW, HW, generator=g)
    torch.save({"clips": clips, "labels": torch.arange(C).repeat(PER), "test_clips": torch.randn(7, T, 3, HW, HW, generator=g),
                "test_labels": torch.randint(0, C, (7,), generator=g)}, d / "toy.pt")
    return {"data": str(d / "toy.pt"), "dir": d}


def test_run_frepo_at_two_ranks_deals_targets_and_evaluation(toy):
    import math
    save, log, out = str(toy["dir"] / "two"), str(toy["dir"] / "two.jsonl"), str(toy["dir"] / "pool")
    _ranks(2, ["run_frepo", "--data_file", toy["data"], "--log_file", log, "--save_path", save, "--eval_seed", "23"])
    lines = [json.loads(l) for l in open(log)]
    steps = [l for l in lines if "Loss" in l]
    assert [l["step"] for l in steps] == [1, 2] and all(math.isfinite(l[k]) for l in steps for k in ("Loss", "ln_loss", "lb_loss"))
    accs = [l for l in lines if "Accuracy/ConvNet3D" in l]
    assert [l["step"] for l in accs] == [1]
    d = os.path.join(save, "Baseline_FRePo", "toy_ipc1_100.0_0.001")          # rank 1's save raises in the tool: these are rank 0's
    best = ["images_best.pt", "y_syn_best.pt"] if accs[0]["Accuracy/ConvNet3D"] > 0 else []
    assert sorted(os.listdir(d)) == sorted(["images_1.pt", "y_syn_1.pt"] + best)
    # the set evaluated before iteration 1 is the one saved at iteration 1; its seed is eval_seed + 1
    _ranks(1, ["pool_on", "--data_file", toy["data"], "--syn", os.path.join(d, "images_1.pt"), "--y_syn", os.path.join(d, "y_syn_1.pt"),
               "--eval_seed", "24", "--out", out])
    want = json.load(open(out + ".rank0.json"))
    assert want["assignment"] == {"train": [0, 0], "test": [[0], [0]]} and want["test_clips"] == [7, 7]
    print("two ranks: accuracy %r std %r; one rank: per network %r" % (accs[0]["Accuracy/ConvNet3D"], accs[0]["Std/ConvNet3D"], want["acc_test"]))
    assert accs[0]["Accuracy/ConvNet3D"] == want["mean"] and accs[0]["Std/ConvNet3D"] == want["std"]
    assert accs[0]["Max_Accuracy/ConvNet3D"] == max(want["mean"], 0.0)
    assert all(math.isfinite(v) and v > 0 for v in want["loss_test"])


def test_preload_at_one_rank_keeps_the_clips_on_the_device(toy, monkeypatch):
    from video_distillation_amd import frepo, run_frepo
    seen = []
    real_step = frepo.FRePoTrainer.step

    def spy(self, x_target, y_target, *rest, **kw):
        seen.append((x_target.is_cuda, y_target.is_cuda, x_target.detach().cpu(), y_target.detach().cpu()))
        return real_step(self, x_target, y_target, *rest, **kw)
    monkeypatch.setattr(frepo.FRePoTrainer, "step", spy)
    log = []
    argv = ["--memories", "images", "--init", "noise", "--dataset", "toy", "--data_file", toy["data"], "--save_path", str(toy["dir"] / "pre"),
            "--im_size", str(HW), "--frames", str(T), "--Iteration", "2", "--num_nn_state", "2", "--max_online_updates", "4", "--seed", "4",
            "--no_eval", "--train_videos", "preload"]
    run_frepo.run(run_frepo.build_parser().parse_args(argv), log=log)
    assert [r["step"] for r in log if "Loss" in r] == [1, 2] and all(np.isfinite(r["Loss"]) for r in log if "Loss" in r)
    assert len(seen) == 2 and all(a and b for a, b, _, _ in seen)          # the clips never left the device
    blob = torch.load(toy["data"])
    stream = frepo.real_batch_indices(C * PER, run_frepo.REAL_BATCH, torch.Generator().manual_seed(4))
    for _, _, x, y in seen:          # an epoch of six clips is one short batch of 512: the stream's order, epoch after epoch
        idx = next(stream)
        assert sorted(idx.tolist()) == list(range(C * PER))
        assert torch.equal(x, blob["clips"][idx]) and torch.equal(y, frepo.soft_labels(blob["labels"][idx], C))


@pytest.mark.parametrize("size", [None, 64])
def test_a_resident_batch_equals_the_host_items_under_the_same_draws(size):
    """On the golden frame folders of tests/test_gpu_resident.py: the table rank 0 draws, sent as int64 rows and turned back into
    draws, gives the clips ``dataset[i]`` gives under the same generator state, bit for bit, and leaves the generators alike."""
    from video_distillation_amd import dataset as D, frepo, run_frepo
    make = (lambda: D.UCF101(UCF, "train")) if size is None else (lambda: D.UCF101(UCF, "train", D.FrameTransform((size, size))))
    ds = make()
    videos = D.ResidentVideos.from_dataset(ds, "cuda:0")
    num_classes = int(max(ds.labels)) + 1
    store = run_frepo.RealStore(num_classes, videos=videos)
    assert store.width == 2 + 3 * D.NUM_FRAMES and store.n == len(ds)
    order = next(frepo.real_batch_indices(store.n, 512, torch.Generator().manual_seed(1)))

    def seed():
        np.random.seed(5); random.seed(7); torch.manual_seed(3)
    seed()
    rows = store.table(order)
    after = (np.random.randint(1 << 30), random.random(), int(torch.randint(1 << 30, (1,))))
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (store.n, store.width)
    wire = rows.clone().reshape(-1).reshape(rows.shape)          # what the broadcast carries
    clips = store.clips(wire)
    labels = store.labels(wire)
    host = make()
    seed()
    want = [host[videos.indices[k]] for k in order.tolist()]
    assert after == (np.random.randint(1 << 30), random.random(), int(torch.randint(1 << 30, (1,))))
    assert clips.is_cuda and torch.equal(clips.cpu().view(torch.int32), torch.stack([w[0] for w in want]).float().view(torch.int32))
    assert torch.equal(labels.cpu(), frepo.soft_labels(torch.tensor([int(w[1]) for w in want]), num_classes))
    lo, hi = frepo.rank_slice(store.n, 1, 2)          # a rank's slice of the table gives its rows of the batch
    assert torch.equal(store.clips(wire[lo:hi]), clips[lo:hi])
