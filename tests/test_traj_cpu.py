"""The argument checks of the ``vdt_`` entry points without a GPU (their declarations and binding: tests/test_cabi.py), the
numpy oracle of the chain against plain fp64, ``experts.ExpertStore`` on the CPU (rows, walks, refusals) and ``MTTTrainer.step`` fed from a ``FlatTrajectory`` against the list form (oracle ops; C = 3, 64x64x8)."""
import math
import os
import random

import numpy as np
import pytest
import torch

from tests import traj_oracle as O
from video_distillation_amd import checkpoint, distill, experts, hip

C = 3


# ---- ABI --------------------------------------------------------------------------------------------------------------

def test_argument_errors_come_back_as_codes_before_any_device_call():
    """Null, misaligned (4 bytes off) and n <= 0: -1 / -2 as in include/vd_hip.h, with no GPU in the machine.  The addresses
    are never dereferenced on these paths."""
    lib = hip.lib()
    a = 0x10000          # "aligned" stand-ins: six distinct multiples of 16
    A = [a + 0x1000 * k for k in range(9)]
    assert lib.vdt_traj_scratch_doubles(0) == 0 and lib.vdt_traj_scratch_doubles(-5) == 0
    assert lib.vdt_traj_scratch_doubles(1) == 2 and lib.vdt_traj_scratch_doubles(1028) == 4
    assert lib.vdt_traj_scratch_doubles(3641603) == lib.vdt_traj_scratch_doubles(1 << 40) == 2 * 2048          # the capped grid
    step = lambda **k: lib.vdt_traj_step(*[k.get(n, A[j]) for j, n in enumerate(("theta", "g", "lr", "n", "out"))], None)   # noqa: E731
    assert step(n=0) == -2 and step(n=-1) == -2
    for name in ("theta", "g", "lr", "out"):
        assert step(n=8, **{name: None}) == -1, name
        assert step(n=8, **{name: a + 4}) == -1, name
    loss = lambda **k: lib.vdt_traj_loss(*[k.get(n, A[j]) for j, n in enumerate(("theta", "theta0", "target", "n", "scratch", "out", "tbar"))], None)   # noqa: E731
    assert loss(n=0) == -2
    for name in ("theta", "theta0", "target", "scratch", "out", "tbar"):
        assert loss(n=8, **{name: None}) == -1, name
        assert loss(n=8, **{name: a + 4}) == -1, name
    names = ("tbar", "hv", "g", "lr", "share", "n", "scratch", "g_lr", "v")
    adj = lambda **k: lib.vdt_traj_adjoint(*[k.get(n, 0.5 if n == "share" else A[j]) for j, n in enumerate(names)], None)   # noqa: E731
    assert adj(n=0) == -2 and adj(n=0, hv=None) == -2
    for name in ("tbar", "g", "lr", "scratch", "g_lr", "v"):
        assert adj(n=8, **{name: None}) == -1, name
        assert adj(n=8, **{name: a + 4}) == -1, name
    assert adj(n=8, hv=a + 4) == -1          # hv may be null, not misaligned
    assert adj(n=8, hv=a + 8) == -1
    with pytest.raises(RuntimeError, match=r"^vdt_traj_step failed with code -2$"):
        hip.run("vdt_traj_step", A[0], A[1], A[2], 0, A[4], None)


# ---- the oracle against plain fp64 ---------------------------------------------------------------------------------------

def test_oracle_restates_the_formulas():
    g = np.random.default_rng(3)
    n = 1029
    theta, theta0, target, grad, hv = (g.normal(0, 0.05, n).astype(np.float32) for _ in range(5))
    lr, share = np.float32(0.0123), 0.75
    out = O.traj_step(theta, grad, lr)
    assert out.dtype == np.float32
    np.testing.assert_allclose(out, theta.astype(np.float64) - float(lr) * grad.astype(np.float64), rtol=0, atol=1e-8)
    assert np.array_equal(out, (torch.tensor(theta) - torch.tensor(lr) * torch.tensor(grad)).numpy())      # the trainer's torch expression
    dist, dist0 = O.traj_dists(theta, theta0, target)
    assert abs(dist / float(((theta.astype(np.float64) - target) ** 2).sum()) - 1) < 1e-13
    assert abs(dist0 / float(((theta0.astype(np.float64) - target) ** 2).sum()) - 1) < 1e-13
    tbar = O.traj_tbar(theta, target, dist0)
    assert np.array_equal(tbar, (2.0 * (torch.tensor(theta) - torch.tensor(target)) / torch.tensor(np.float32(dist0))).numpy())
    t2, dot, dot_abs, v = O.traj_adjoint(tbar, hv, grad, lr, share)
    assert np.array_equal(t2, tbar + hv) and dot_abs >= abs(dot)
    assert abs(dot - float((t2.astype(np.float64) * grad).sum())) < 1e-12 * dot_abs
    assert np.array_equal(v, (torch.tensor(t2) * (-torch.tensor(lr) * share)).numpy())
    t3, _, _, _ = O.traj_adjoint(tbar, None, grad, lr, share)
    assert np.array_equal(t3, tbar)


# ---- ExpertStore on the CPU ----------------------------------------------------------------------------------------------

def _random_walk(gen, experts_n, epochs, num_classes=C):
    out = []
    for _ in range(experts_n):
        cur = [0.05 * torch.randn(s, generator=gen) for s in distill.FULL_SHAPES(num_classes)]
        traj = [cur]
        for _ in range(epochs - 1):
            cur = [p + 0.01 * p.abs().mean() * torch.randn(p.shape, generator=gen) for p in cur]
            traj.append(cur)
        out.append(traj)
    return out


@pytest.fixture(scope="module")
def buffers(tmp_path_factory):
    d = tmp_path_factory.mktemp("buffers")
    gen = torch.Generator().manual_seed(77)
    files = [_random_walk(gen, 3, 4), _random_walk(gen, 2, 4)]
    for f in files:
        checkpoint.save_expert_buffer(str(d), f)
    return {"dir": str(d), "files": files}


def test_store_discovers_files_like_the_loader(buffers, tmp_path):
    with pytest.raises(AssertionError, match="No buffers detected"):
        experts.ExpertStore(str(tmp_path), C, "cpu")
    assert [os.path.basename(f) for f in experts.buffer_files(buffers["dir"])] == ["replay_buffer_0.pt", "replay_buffer_1.pt"]
    assert len(experts.buffer_files(buffers["dir"], max_files=1)) == 1
    assert experts.param_count(C) == 3641603 and experts.padded(3641603) == 3641604          # P is odd at C = 3


@pytest.mark.parametrize("mode", ["host", "resident"])
def test_rows_are_the_flattened_tensors_of_the_files(buffers, mode):
    store = experts.ExpertStore(buffers["dir"], C, "cpu", mode=mode, walk="all", seed=5)
    assert store.P == 3641603 and store.Ppad % 4 == 0 and store.epochs == 4
    seen = set()
    for _ in range(5):
        traj = store.next()
        f, e = store.last
        seen.add((f, e))
        assert traj.epochs == 4 and len(traj) == 4
        for epoch in (0, 3):
            row = traj.row(epoch)
            assert row.dtype == torch.float32 and tuple(row.shape) == (store.P,) and row.data_ptr() % 16 == 0
            assert torch.equal(row, distill.flatten_params(buffers["files"][f][e][epoch]))
        assert traj.row(0).data_ptr() != traj.row(3).data_ptr()          # two rows of an iteration are valid together
        with pytest.raises(IndexError):
            traj.row(4)
    assert seen == {(0, 0), (0, 1), (0, 2), (1, 0), (1, 1)}          # one pass of walk="all" visits every expert once


def _walk_restated(sizes, seed, walk, count):
    """The order in ten lines: files shuffled; the current file's experts shuffled and yielded; at the end of a file the next
    one (all) or the same one again (reference: ``file_idx`` moves, nothing is loaded); the files reshuffled after the last."""
    rng = random.Random(seed)
    files = list(range(len(sizes))); rng.shuffle(files)
    pos, cur = 0, files[0]
    order = list(range(sizes[cur])); rng.shuffle(order)
    out = []
    while len(out) < count:
        for e in order:
            out.append((cur, e))
        pos += 1
        if pos == len(files):
            pos = 0; rng.shuffle(files)
        cur = files[pos] if walk == "all" else cur
        order = list(range(sizes[cur])) if walk == "all" else order
        rng.shuffle(order)
    return out[:count]


@pytest.mark.parametrize("walk", ["all", "reference"])
@pytest.mark.parametrize("mode", ["host", "resident"])
def test_walks_equal_their_restatement(buffers, walk, mode):
    for seed in (0, 1, 9):
        store = experts.ExpertStore(buffers["dir"], C, "cpu", mode=mode, walk=walk, seed=seed)
        got = []
        for _ in range(12):
            store.next()
            got.append(store.last)
        assert got == _walk_restated([3, 2], seed, walk, 12), (walk, seed)
        again = experts.ExpertStore(buffers["dir"], C, "cpu", mode=mode, walk=walk, seed=seed)
        assert [(again.next(), again.last)[1] for _ in range(12)] == got          # the same seed, the same sequence
        if walk == "reference":
            assert len({f for f, _ in got}) == 1          # only the first shuffled file is ever used
        else:
            assert {f for f, _ in got} == {0, 1}
    assert len({tuple(_walk_restated([3, 2], s, "all", 12)) for s in range(6)}) > 1          # (the seed matters)


def test_store_refusals_name_the_numbers(buffers, tmp_path):
    with pytest.raises(ValueError, match=r"3641603 parameters in 8 tensors; --num_classes 5 needs 3641861"):
        experts.ExpertStore(buffers["dir"], 5, "cpu")
    gen = torch.Generator().manual_seed(1)
    uneven = _random_walk(gen, 2, 3)
    uneven[1] = uneven[1][:2]
    checkpoint.save_expert_buffer(str(tmp_path), uneven)
    for mode in ("host", "resident"):
        with pytest.raises(ValueError, match=r"expert 1 holds 2 epochs, expert 0 holds 3"):
            experts.ExpertStore(str(tmp_path), C, "cpu", mode=mode)
    store = experts.ExpertStore(buffers["dir"], C, "cpu")
    store.check(3, 1)          # reads epoch 3 at most: the last row
    store.check(1, 3)
    with pytest.raises(ValueError, match=r"--max_start_epoch 4 --expert_epochs 1 reads epoch 4 of trajectories that hold epochs 0\.\.3"):
        store.check(4, 1)
    with pytest.raises(ValueError, match=r"reads epoch 27"):
        store.check(25, 3)          # the reference's defaults on a 4-epoch buffer: IndexError in the middle of a run there
    with pytest.raises(ValueError, match="mode"):
        experts.ExpertStore(buffers["dir"], C, "cpu", mode="pinned")
    with pytest.raises(ValueError, match="walk"):
        experts.ExpertStore(buffers["dir"], C, "cpu", walk="first")


# ---- trainer: a FlatTrajectory is the list form, without the copies ---------------------------------------------------------

def test_step_from_a_flat_trajectory_equals_the_list_form_and_train_lr_off_keeps_syn_lr(buffers):
    from tests.cpu_backend import OracleMTTOps
    assert not hasattr(OracleMTTOps(), "flat")
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    g = torch.Generator().manual_seed(12)
    image_syn = torch.randn(C, 8, 3, 64, 64, generator=g)
    labels = torch.arange(C)
    chunks = [torch.tensor([2, 0, 1]), torch.tensor([1, 2, 0])]

    def trainer(**kw):
        return distill.MTTTrainer(OracleMTTOps(), C, image_syn.clone(), labels, 0.01, lr_img=100.0, lr_lr=1e-3, syn_steps=2,
                                  batch_syn=3, expert_epochs=2, max_start_epoch=2, **kw)
    store = experts.ExpertStore(buffers["dir"], C, "cpu", mode="host", walk="all", seed=2)
    traj = store.next()
    f, e = store.last
    a = trainer()
    grand_a = a.step(0, buffers["files"][f][e], start_epoch=1, index_chunks=chunks, update=False)
    b = trainer(train_lr=False)
    grand_b = b.step(0, traj, start_epoch=1, index_chunks=chunks)
    assert math.isfinite(float(grand_a)) and float(grand_a) == float(grand_b)
    assert torch.equal(a.last_grads[0], b.last_grads[0]) and torch.equal(a.last_grads[1], b.last_grads[1])
    assert b.last_grads[1].dim() == 0 and b.last_grads[1].dtype == torch.float32 and float(b.last_grads[1]) != 0.0
    assert a.last_start_epoch == b.last_start_epoch == 1
    # train_lr=False: the clips are stepped, syn_lr and its momentum are not
    assert float(b.syn_lr) == float(torch.tensor(0.01, dtype=torch.float32)) and float(b.lr_buf) == 0.0 and b.steps_done == 1
    assert not torch.equal(b.image_syn, image_syn) and torch.equal(a.image_syn, image_syn)
    assert a.train_lr and not b.train_lr          # (the default steps syn_lr: tests/test_distributed_cpu.py pins that update)
