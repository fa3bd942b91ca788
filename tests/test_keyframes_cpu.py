"""Key-frame memories without a GPU: ``keyframes.table``, the argument checks of the three ``vdk_`` entry points
(include/vd_keyframes.h; its binding, layout and hashes: tests/test_cabi.py), the torch expressions of expand / reduce against host loops of ``np.float32`` operations,
``distill.KeyframeDMTrainer`` on ``tests.cpu_backend.OracleBackend`` (K = T against ``DMTrainer`` bit for bit, three steps against
float64 autograd, two gloo ranks against one) and ``run_dm --memories keyframes`` on the oracle backend.

The host loops ``np_expand`` / ``np_reduce`` here are the bitwise reference of tests/test_gpu_keyframes.py too."""
import ctypes
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as R
from tests.cpu_backend import OracleBackend
from video_distillation_amd import checkpoint, distill, hip, keyframes, plan, run_dm

C, IPC, T, HW, PER, BATCH = 2, 2, 8, 64, 12, 8
LR, MU, STEPS = 0.1, 0.5, 3
SEED = 5151
TABLES = [(1, 1, "linear"), (8, 1, "linear"), (5, 2, "linear"), (8, 3, "linear"), (16, 4, "linear"), (16, 16, "linear"),
          (8, 3, "nearest"), (16, 4, "nearest")]


# ---- the host loops: one np.float32 operation per product and per add ------------------------------------------------------

def np_expand(keys, tab):
    """(n, K, ...) float32 -> (n, T, ...): w0 * k0 + w1 * k1, a zero weight's term skipped, each operation rounded to float32."""
    out = np.zeros((keys.shape[0], tab.T) + keys.shape[2:], dtype=np.float32)
    for t in range(tab.T):
        r = None
        for idx, w in ((tab.i0[t], tab.w0[t]), (tab.i1[t], tab.w1[t])):
            if w == 0:
                continue
            p = (np.float32(w) * keys[:, idx]).astype(np.float32)
            r = p if r is None else (r + p).astype(np.float32)
        if r is not None:
            out[:, t] = r
    return out


def np_reduce(g, tab):
    """(n, T, ...) float32 -> (n, K, ...): per key the products of its terms, ascending t, i0 before i1, the accumulator started
    from the first product, 0 for a key without a term."""
    out = np.zeros((g.shape[0], tab.K) + g.shape[2:], dtype=np.float32)
    for k in range(tab.K):
        acc = None
        for t in range(tab.T):
            for idx, w in ((tab.i0[t], tab.w0[t]), (tab.i1[t], tab.w1[t])):
                if w == 0 or idx != k:
                    continue
                p = (np.float32(w) * g[:, t]).astype(np.float32)
                acc = p if acc is None else (acc + p).astype(np.float32)
        if acc is not None:
            out[:, k] = acc
    return out


# ---- table() ---------------------------------------------------------------------------------------------------------------

def test_table_values_at_16_4():
    i0, i1, w0, w1 = keyframes.table(16, 4, "linear")
    assert i0.dtype == i1.dtype == np.int32 and w0.dtype == w1.dtype == np.float32 and all(len(a) == 16 for a in (i0, i1, w0, w1))
    assert i0.tolist() == [0] * 5 + [1] * 5 + [2] * 6 and i1.tolist() == [1] * 5 + [2] * 5 + [3] * 6
    want = [1, .8, .6, .4, .2] * 3 + [0]
    np.testing.assert_allclose(w0, want, atol=2.0 ** -23)
    np.testing.assert_allclose(w1, [1 - v for v in want], atol=2.0 ** -23)
    assert w0[0] == 1 and w1[0] == 0 and w0[5] == 1 and w0[10] == 1 and w0[15] == 0 and w1[15] == 1          # the last frame copies the last key
    tab = keyframes.table(16, 4, "linear")
    assert (tab.T, tab.K, tab.interp) == (16, 4, "linear")
    j0, j1, v0, v1 = keyframes.table(16, 4, "nearest")
    assert j0.tolist() == j1.tolist() == [t // 4 for t in range(16)] and (v0 == 1).all() and (v1 == 0).all()


@pytest.mark.parametrize("interp", ["linear", "nearest"])
def test_table_ends_identity_and_still_and_weights_sum_to_one(interp):
    for T_ in (1, 2, 5, 8, 16, 64):
        tab = keyframes.table(T_, T_, interp)          # K = T: one weight of exactly 1 per frame, on key t
        for t in range(T_):
            terms = [(int(i), float(w)) for i, w in ((tab.i0[t], tab.w0[t]), (tab.i1[t], tab.w1[t])) if w != 0]
            assert terms == [(t, 1.0)], (T_, t)
        one = keyframes.table(T_, 1, interp)          # K = 1: all ones on key 0
        assert not one.i0.any() and not one.i1.any() and (one.w0 == 1).all() and (one.w1 == 0).all()
        for K in range(1, T_ + 1):
            tab = keyframes.table(T_, K, interp)
            assert (np.abs(tab.w0.astype(np.float64) + tab.w1.astype(np.float64) - 1.0) <= 2.0 ** -24).all()
            assert tab.i0.min() >= 0 and tab.i1.max() <= K - 1 and (tab.w0 >= 0).all() and (tab.w1 >= 0).all()
            assert all(tab.terms(k) for k in range(K)), (T_, K)          # every key is used
            assert hip.lib().vdk_table_check(ctypes.addressof(hip.vdk_table(tab))) == 0


def test_table_refusals():
    for bad in ((8, 0, "linear"), (8, -1, "nearest"), (8, 9, "linear"), (65, 4, "linear"), (65, 65, "nearest"), (8, 4, "cubic"),
                (8, 4, ""), (0, 0, "linear")):
        with pytest.raises(ValueError):
            keyframes.table(*bad)
    with pytest.raises(ValueError):
        keyframes.table(1, 2, "linear")
    assert keyframes.table(1, 1, "linear").w0.tolist() == [1.0] and keyframes.table(64, 64, "linear").T == 64


@pytest.mark.parametrize("T_,K", [(5, 2), (8, 3), (16, 4), (16, 16), (64, 7), (2, 2)])
def test_linear_table_is_interpolate_align_corners(T_, K):
    g = torch.Generator().manual_seed(T_ * 100 + K)
    keys = torch.rand(3, K, 3, 4, 5, generator=g, dtype=torch.float64) * 2 - 1
    got = keyframes.expand_torch(keys, keyframes.table(T_, K, "linear"))
    flat = keys.permute(0, 2, 3, 4, 1).reshape(1, -1, K)
    want = torch.nn.functional.interpolate(flat, size=T_, mode="linear", align_corners=True).reshape(3, 3, 4, 5, T_).permute(0, 4, 1, 2, 3)
    assert float((got - want).abs().max()) <= 1e-6


# ---- ABI --------------------------------------------------------------------------------------------------------------------

def _ctable(T_=8, K=3, interp="linear"):
    """A fresh ``hip.VdkTable`` of its own (not the mirror a ``keyframes.Table`` keeps), free to be broken."""
    src = hip.vdk_table(keyframes.table(T_, K, interp))
    c = hip.VdkTable()
    ctypes.memmove(ctypes.addressof(c), ctypes.addressof(src), ctypes.sizeof(c))
    return c


def test_table_check():
    lib = hip.lib()
    assert lib.vdk_table_check(None) == -1
    c = _ctable()          # (kept in a name: the address of a temporary outlives it)
    assert lib.vdk_table_check(ctypes.addressof(c)) == 0
    for field, value in (("T", 0), ("T", 65), ("T", -1), ("K", 0), ("K", 9), ("K", -3)):
        c = _ctable()
        setattr(c, field, value)
        assert lib.vdk_table_check(ctypes.addressof(c)) == -1, (field, value)
    c = _ctable(64, 64)
    assert lib.vdk_table_check(ctypes.addressof(c)) == 0
    for arr, value in (("i0", -1), ("i0", 3), ("i1", 3), ("i1", -1), ("w0", float("inf")), ("w1", float("nan")), ("w0", float("-inf"))):
        for t in (0, 7):
            c = _ctable()
            getattr(c, arr)[t] = value
            assert lib.vdk_table_check(ctypes.addressof(c)) == -1, (arr, value, t)
        c = _ctable()
        getattr(c, arr)[8] = value          # entries at t >= T are not read
        assert lib.vdk_table_check(ctypes.addressof(c)) == 0
    c = _ctable()
    c.w0[2], c.w1[2] = -3.5, 0.0          # any finite weight passes
    assert lib.vdk_table_check(ctypes.addressof(c)) == 0


def test_argument_errors_come_back_as_codes_before_any_device_call():
    """-1 for a bad table, a non-positive H / W or a negative n; then 0 for n == 0; then -1 for a null data pointer -- with null
    streams and no GPU in the machine.  The addresses are never dereferenced on these paths."""
    lib = hip.lib()
    A = [0x10000 + 0x1000 * k for k in range(3)]
    good, bad = _ctable(), _ctable()
    bad.i1[3] = 3
    tab = ctypes.addressof(good)
    for fn in (lib.vdk_keyframe_expand, lib.vdk_keyframe_reduce):
        call = lambda src=A[0], n=3, table=tab, H=5, W=7, dst=A[1]: fn(src, n, table, H, W, dst, None)          # noqa: E731
        for dim in ("H", "W"):
            assert call(**{dim: 0}) == -1 and call(**{dim: -2}) == -1
            assert call(n=0, **{dim: 0}) == -1          # (the shape is checked before the empty batch is let through)
        assert call(table=None) == -1 and call(table=ctypes.addressof(bad)) == -1
        assert call(table=None, n=0) == -1 and call(table=ctypes.addressof(bad), n=0) == -1
        assert call(n=-1) == -1
        assert call(n=0) == 0 and call(n=0, src=None, dst=None) == 0
        assert call(src=None) == -1 and call(dst=None) == -1
    with pytest.raises(RuntimeError, match=r"^vdk_keyframe_reduce failed with code -1$"):
        hip.run("vdk_keyframe_reduce", A[0], 3, tab, 0, 7, A[1], None)


def test_python_wrappers_refuse_before_the_kernel():
    tab = keyframes.table(8, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.keyframe_expand(torch.zeros(2, 3, 3, 5, 7), tab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.keyframe_reduce(torch.zeros(2, 8, 3, 5, 7), tab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.keyframe_expand(torch.zeros(2, 3, 3, 5, 7, dtype=torch.float64), tab)
    for bad in (torch.zeros(2, 4, 3, 5, 7), torch.zeros(2, 3, 1, 5, 7), torch.zeros(3, 3, 5, 7), torch.zeros(2, 3, 3, 0, 7)):
        with pytest.raises(ValueError):
            hip.keyframe_expand(bad, tab)
    for bad in (torch.zeros(2, 3, 3, 5, 7), torch.zeros(2, 8, 2, 5, 7), torch.zeros(8, 3, 5, 7)):
        with pytest.raises(ValueError):
            hip.keyframe_reduce(bad, tab)
    broken = keyframes.table(8, 3)
    broken.i1[2] = 3
    with pytest.raises(ValueError, match="index outside"):
        hip.keyframe_expand(torch.zeros(2, 3, 3, 5, 7), broken)
    assert isinstance(hip.vdk_table(tab), hip.VdkTable) and hip.vdk_table(tab) is hip.vdk_table(tab)


# ---- the torch expressions the CPU oracle backend takes --------------------------------------------------------------------

@pytest.mark.parametrize("T_,K,interp", TABLES)
def test_torch_expressions_equal_the_float32_host_loops_and_are_adjoint(T_, K, interp):
    be = OracleBackend()
    assert not hasattr(be, "keyframe_expand") and not hasattr(be, "keyframe_reduce")
    tab = keyframes.table(T_, K, interp)
    rng = np.random.default_rng(100 * T_ + K)
    keys = (rng.normal(0, 1, (3, K, 3, 5, 7)) * 10.0 ** rng.integers(-3, 3, (3, K, 1, 1, 1))).astype(np.float32)
    g = (rng.normal(0, 1, (3, T_, 3, 5, 7)) * 10.0 ** rng.integers(-3, 3, (3, T_, 1, 1, 1))).astype(np.float32)
    e = distill.keyframe_expand(be, torch.from_numpy(keys), tab)
    r = distill.keyframe_reduce(be, torch.from_numpy(g), tab)
    assert e.shape == (3, T_, 3, 5, 7) and r.shape == (3, K, 3, 5, 7) and e.is_contiguous() and r.is_contiguous()
    assert np.array_equal(e.numpy().view(np.uint32), np_expand(keys, tab).view(np.uint32))
    assert np.array_equal(r.numpy().view(np.uint32), np_reduce(g, tab).view(np.uint32))
    k64, g64 = torch.from_numpy(keys).double(), torch.from_numpy(g).double()
    lhs = float((keyframes.expand_torch(k64, tab) * g64).sum())
    rhs = float((k64 * keyframes.reduce_torch(g64, tab)).sum())
    assert abs(lhs - rhs) <= 1e-6 * max(abs(lhs), abs(rhs))
    if K == 1:          # the still clip
        assert torch.equal(e, distill.still_expand(be, torch.from_numpy(keys[:, 0]), None, T_))
        assert torch.equal(r[:, 0], distill.still_reduce(be, torch.from_numpy(g)))
    if K == T_:
        assert torch.equal(e, torch.from_numpy(keys)) and torch.equal(r, torch.from_numpy(g))


# ---- the trainer -----------------------------------------------------------------------------------------------------------

def keyframe_case():
    """The inputs of the trainer tests here and in tests/test_gpu_keyframes.py: 12 clips per class; the network of iteration
    ``it`` is the oracle's of seed ``it`` (``OracleBackend.new_network``)."""
    g = torch.Generator().manual_seed(SEED)
    return torch.randn(C * PER, T, 3, HW, HW, generator=g)


def keyframe_trainer(be, dev, clips, K, interp, keys=None, **kw):
    pool = distill.RealPool(clips.to(dev), [PER] * C, [c * PER for c in range(C)])
    return distill.KeyframeDMTrainer(be, pool, plan.NetGeometry(T, HW, HW), C, IPC, BATCH, LR, key_frames=K, interp=interp, momentum=MU,
                                     keys=None if keys is None else keys.clone().to(dev), **kw)


def test_k_equal_t_is_the_clip_trainer_bit_for_bit():
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    clips = keyframe_case()
    pool = distill.RealPool(clips, [PER] * C, [c * PER for c in range(C)])
    ref = distill.DMTrainer(OracleBackend(), pool, C, IPC, BATCH, LR, momentum=MU)
    tr = keyframe_trainer(OracleBackend(), "cpu", clips, T, "linear")
    assert torch.equal(tr.keys, ref.image_syn) and tr.keys.shape == (C * IPC, T, 3, HW, HW)
    for it in range(STEPS):
        a, b = float(ref.step(it)), float(tr.step(it))
        assert a == b, it
        assert torch.equal(tr.keys, ref.image_syn) and torch.equal(tr.image_syn, ref.image_syn) and torch.equal(tr.buf, ref.buf), it
    assert not torch.equal(tr.keys, clips[[0, 1, PER, PER + 1]])
    assert tr.gather_keys() is tr.keys and torch.equal(tr.gather_syn(), tr.image_syn)


def autograd_dm_step(it, clips, keys, tab, dtype):
    """Iteration ``it`` of the DM loss in plain autograd on the oracle net, the synthetic clips the two-tap combination of
    ``keys`` -> (loss, d loss / d keys)."""
    params = [p.to(dtype) for p in R.init_params(it)[:6]] + [None, None]
    idx = distill.sample_real_indices(it, [PER] * C, [c * PER for c in range(C)], BATCH, list(range(C)))
    with torch.no_grad():
        f_real = R.convnet3d_embed(clips[torch.as_tensor(idx)].to(dtype), params)
    kv = keys.to(dtype).clone().requires_grad_(True)
    frames = [float(tab.w0[t]) * kv[:, int(tab.i0[t])] + float(tab.w1[t]) * kv[:, int(tab.i1[t])] for t in range(tab.T)]
    f_syn = R.convnet3d_embed(torch.stack(frames, 1), params)
    d = f_real.shape[1]
    loss = (((f_real.view(C, -1, d).mean(1) - f_syn.view(C, -1, d).mean(1)) ** 2).sum(1)).sum()
    loss.backward()
    return float(loss.detach()), kv.grad.detach()


_ORACLE_RUNS = {}


def oracle_steps(K, interp):
    """Three steps of the key-frame trainer on the fp32 oracle backend (computed once per table; shared with the GPU tests)."""
    if (K, interp) not in _ORACLE_RUNS:
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
        clips = keyframe_case()
        tr = keyframe_trainer(OracleBackend(), "cpu", clips, K, interp)
        keys0 = tr.keys.clone()
        losses = [float(tr.step(it)) for it in range(STEPS)]
        _ORACLE_RUNS[(K, interp)] = dict(clips=clips, keys0=keys0, losses=losses, keys=tr.keys.clone(), tr=tr)
    return _ORACLE_RUNS[(K, interp)]


@pytest.mark.parametrize("K,interp", [(3, "linear"), (2, "nearest")])
def test_three_steps_are_finite_and_the_fp32_oracle_is_well_inside_the_gpu_bars_against_fp64(K, interp):
    """tests/test_gpu_keyframes.py compares HIP with this fp32 oracle run (loss 1e-3 relative at every step, key update 5e-2
    rel-l2 per class).  The fp32 oracle itself stays at least ten times inside both bars against the same three steps,
    momentum included, in float64 autograd through the two-tap combination."""
    run = oracle_steps(K, interp)
    tr, keys0 = run["tr"], run["keys0"]
    tab = keyframes.table(T, K, interp)
    assert keys0.shape == (C * IPC, K, 3, HW, HW) and tr.buf.shape == keys0.shape and tr.steps_done == STEPS
    assert all(np.isfinite(run["losses"])) and bool(torch.isfinite(tr.keys).all()) and not torch.equal(tr.keys, keys0)
    assert torch.equal(tr.image_syn, keyframes.expand_torch(tr.keys, tab))          # the next step's clips
    picks = keyframes.init_frames(T, K, interp)
    assert torch.equal(keys0, run["clips"][[0, 1, PER, PER + 1]][:, picks])
    keys, buf, rel_loss = keys0.double(), None, []
    for it in range(STEPS):
        loss64, g64 = autograd_dm_step(it, run["clips"], keys, tab, torch.float64)
        buf = g64 if buf is None else MU * buf + g64
        keys = keys - LR * buf
        rel_loss.append(abs(run["losses"][it] - loss64) / abs(loss64))
    up32, up64 = tr.keys.double() - keys0.double(), keys - keys0.double()
    per = [float((up32[c * IPC:(c + 1) * IPC] - up64[c * IPC:(c + 1) * IPC]).norm() / up64[c * IPC:(c + 1) * IPC].norm()) for c in range(C)]
    print("K %d %s: fp32 oracle vs float64, %d steps: loss rel %s, key update rel-l2 per class %s"
          % (K, interp, STEPS, ["%.3e" % e for e in rel_loss], ["%.3e" % e for e in per]))
    assert max(rel_loss) < 1e-4 and max(per) < 5e-3


def test_trainer_refusals_hooks_and_init_real():
    geo = plan.NetGeometry(T, HW, HW)
    be = OracleBackend()
    clips = (torch.arange(6.).view(6, 1, 1, 1, 1) * 100 + torch.arange(float(T)).view(1, T, 1, 1, 1)).expand(6, T, 3, HW, HW).contiguous()
    pool = distill.RealPool(clips, [3, 3], [0, 3])
    with pytest.raises(ValueError, match="pool of clips"):
        distill.KeyframeDMTrainer(be, distill.RealPool(clips[:, 0], [3, 3], [0, 3]), geo, 2, 2, 1, 0.1)
    with pytest.raises(ValueError, match="allreduce"):
        distill.KeyframeDMTrainer(be, pool, geo, 2, 2, 1, 0.1, exchange="allreduce")
    with pytest.raises(ValueError, match="keys"):
        distill.KeyframeDMTrainer(be, pool, geo, 2, 2, 1, 0.1, key_frames=3, keys=torch.zeros(4, 4, 3, HW, HW))
    for K, interp in ((0, "linear"), (T + 1, "linear"), (2, "cubic")):
        with pytest.raises(ValueError):
            distill.KeyframeDMTrainer(be, pool, geo, 2, 2, 1, 0.1, key_frames=K, interp=interp)
    # --init real: the first ipc clips of each class; key k from frame (k*(T-1) + (K-1)//2) // (K-1) (linear) or (k*T + K-1) // K
    assert keyframes.init_frames(8, 3, "linear") == [0, 4, 7] and keyframes.init_frames(8, 3, "nearest") == [0, 3, 6]
    assert keyframes.init_frames(16, 4, "linear") == [0, 5, 10, 15] and keyframes.init_frames(16, 4, "nearest") == [0, 4, 8, 12]
    assert keyframes.init_frames(8, 1, "linear") == [0] == keyframes.init_frames(8, 1, "nearest")
    assert keyframes.init_frames(8, 8, "linear") == list(range(8)) == keyframes.init_frames(8, 8, "nearest")
    for interp, frames in (("linear", [0, 4, 7]), ("nearest", [0, 3, 6])):
        tr = distill.KeyframeDMTrainer(be, pool, geo, 2, 2, 1, 0.1, key_frames=3, interp=interp)
        assert tr.keys[:, :, 0, 0, 0].tolist() == [[c + f for f in frames] for c in (0.0, 100.0, 300.0, 400.0)]
        assert tr.image_syn.shape == (4, T, 3, HW, HW) and tr.buf.shape == tr.keys.shape and not tr.buf.any() and tr.ipc == 2
    assert distill.KeyframeDMTrainer.step is distill.DMTrainer.step and distill.KeyframeDMTrainer._embed_real is distill.DMTrainer._embed_real
    assert distill.KeyframeDMTrainer._flush_backward is distill.DMTrainer._flush_backward
    assert distill.KeyframeDMTrainer._apply_pixel_grad is not distill.DMTrainer._apply_pixel_grad


# ---- sharding: two ranks reproduce one -------------------------------------------------------------------------------------

def _dm_run(rank, world, shard):
    clips = keyframe_case()
    tr = keyframe_trainer(OracleBackend(), "cpu", clips, 3, "linear", rank=rank, world=world, shard=shard)
    lo, hi = distill.class_range(C, rank, world)
    assert tr.owned_classes() == list(range(lo, hi)) and tr.keys.shape[0] == (hi - lo) * IPC
    losses = [float(tr.global_loss(tr.step(it))) for it in range(2)]
    return losses, tr.gather_keys(), tr.gather_syn()


def _worker_dm(rank, world, port, q, shard):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        losses, keys, syn = _dm_run(rank, world, shard)
        if rank == 0:
            q.put((losses, keys.numpy(), syn.numpy()))
    finally:
        dist.destroy_process_group()


def _worker_dm_class(rank, world, port, q):
    _worker_dm(rank, world, port, q, "class")


def _worker_dm_batch(rank, world, port, q):
    _worker_dm(rank, world, port, q, "batch")


@pytest.fixture(scope="module")
def one_rank_run():
    torch.set_num_threads(4)
    return _dm_run(0, 1, "class")


@pytest.mark.parametrize("worker", [_worker_dm_class, _worker_dm_batch], ids=["class", "batch"])
def test_keyframe_trainer_sharding_identity_two_ranks_gloo(worker, one_rank_run):
    """Two steps on two ranks -- one class each ('class'), or half of every class's real batch each with the feature sums
    all-reduced ('batch') -- reproduce the one-rank run: summed loss, gathered keys in class order, gathered clips = their
    expansion.  Bars: the identity bars of tests/test_distributed_cpu.py (loss rtol 2e-5; memories rtol 1e-4, atol 1e-6)."""
    from tests.test_distributed_cpu import _spawn
    want_l, want_k, _ = one_rank_run
    got_l, got_k, got_s = _spawn(worker, 2)
    np.testing.assert_allclose(got_l, want_l, rtol=2e-5)
    np.testing.assert_allclose(got_k, want_k.numpy(), rtol=1e-4, atol=1e-6)
    assert got_k.shape == (C * IPC, 3, 3, HW, HW) and got_s.shape == (C * IPC, T, 3, HW, HW)
    assert np.array_equal(got_s, np_expand(got_k, keyframes.table(T, 3, "linear")))
    assert not np.allclose(want_k.numpy(), keyframe_case()[[0, 1, PER, PER + 1]][:, [0, 4, 7]].numpy())


# ---- the driver and the files ----------------------------------------------------------------------------------------------

def _args(tmp_path, *extra):
    return run_dm.build_parser().parse_args([
        "--memories", "keyframes", "--dataset", "synthetic", "--num_classes", "2", "--pool_per_class", "3", "--ipc", "2", "--Iteration", "1",
        "--batch_real", "2", "--frames", "8", "--im_size", "64", "--lr_img", "0.1", "--eval_it", "2", "--num_eval", "1",
        "--epoch_eval_train", "1", "--batch_train", "4", "--save_path", str(tmp_path)] + list(extra))


def test_flags_of_the_keyframe_mode():
    args = run_dm.build_parser().parse_args([])
    assert (args.memories, args.key_frames, args.interp, args.spc, args.seed, args.ipc, args.frames) == ("images", 4, "linear", 2, 0, 1, 16)
    with pytest.raises(SystemExit):
        run_dm.build_parser().parse_args(["--memories", "s2d"])
    with pytest.raises(SystemExit):
        run_dm.build_parser().parse_args(["--memories", "keyframes", "--interp", "cubic"])


def test_run_dm_keyframes_on_the_oracle_backend(tmp_path):
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    log = []
    args = _args(tmp_path, "--key_frames", "3")
    tr = run_dm.run(args, backend=OracleBackend(), log=log)
    losses = [r["Loss"] for r in log if "Loss" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[0] > 0
    assert type(tr) is distill.KeyframeDMTrainer and tr.steps_done == 2 and (tr.key_frames, tr.interp) == (3, "linear")
    assert tr.keys.shape == (4, 3, 3, 64, 64) and tr.image_syn.shape == (4, 8, 3, 64, 64)
    save_dir = os.path.join(tmp_path, "Keyframes_DM", "synthetic_ipc2_k3_linear_0.1")
    assert sorted(os.listdir(save_dir)) == ["keyframes_0.pt"]          # images' cadence: iteration 0 is a multiple of 1000, no best without test clips
    frames, interp, T_ = checkpoint.load_keyframes(os.path.join(save_dir, "keyframes_0.pt"))
    assert frames.shape == (4, 3, 3, 64, 64) and frames.dtype == torch.float32 and (interp, T_) == ("linear", 8)
    pool = run_dm.load_data(args, 0, 1, plan.NetGeometry(8, 64, 64), torch.device("cpu"))[0]
    assert torch.equal(frames, pool.clips[[0, 1, 3, 4]][:, [0, 4, 7]])          # --init real, saved before the first step
    assert not torch.equal(tr.keys, frames)
    images = checkpoint.keyframes_to_images(os.path.join(save_dir, "keyframes_0.pt"))
    assert images.shape == (4, 8, 3, 64, 64) and torch.equal(images, keyframes.expand_torch(frames, keyframes.table(8, 3, "linear")))
    assert torch.equal(images[:, 0], frames[:, 0]) and torch.equal(images[:, 7], frames[:, 2])
    path = checkpoint.save_keyframes(str(tmp_path / "after"), 7, tr.gather_keys(), tr.interp, 8, best=True)
    assert torch.equal(checkpoint.keyframes_to_images(path), tr.gather_syn())
    assert torch.equal(checkpoint.keyframes_to_images(str(tmp_path / "after" / "keyframes_best.pt")), tr.gather_syn())
    with pytest.raises(ValueError, match="allreduce"):
        run_dm.run(_args(tmp_path), backend=OracleBackend(), log=[], exchange="allreduce")
    with pytest.raises(ValueError):
        run_dm.run(_args(tmp_path, "--key_frames", "9"), backend=OracleBackend(), log=[])
    with pytest.raises(ValueError):
        checkpoint.save_keyframes(str(tmp_path), 0, torch.zeros(4, 3, 64, 64), "linear", 8)
    with pytest.raises(KeyError):
        torch.save({"image": torch.zeros(1)}, str(tmp_path / "other.pt"))
        checkpoint.load_keyframes(str(tmp_path / "other.pt"))


def test_run_dm_keyframes_nearest_noise_comes_from_the_seed(tmp_path):
    args = _args(tmp_path, "--init", "noise", "--seed", "3", "--Iteration", "0", "--key_frames", "2", "--interp", "nearest", "--no_eval")
    tr = run_dm.run(args, backend=OracleBackend(), log=[])
    noise = torch.randn((4, 2, 3, 64, 64), generator=torch.Generator().manual_seed(3))
    assert tr.steps_done == 1 and tr.keys.shape == noise.shape
    assert torch.allclose(tr.keys + LR * tr.buf, noise, rtol=0, atol=1e-6)          # one step from the noise: keys = noise - lr * g
    assert not os.path.exists(os.path.join(tmp_path, "Keyframes_DM"))          # images' cadence: --no_eval writes nothing
    args = _args(tmp_path, "--init", "noise", "--seed", "3", "--Iteration", "0", "--key_frames", "2", "--interp", "nearest")
    run_dm.run(args, backend=OracleBackend(), log=[])
    saved, interp, T_ = checkpoint.load_keyframes(os.path.join(tmp_path, "Keyframes_DM", "synthetic_ipc2_k2_nearest_0.1", "keyframes_0.pt"))
    assert torch.equal(saved, noise) and (interp, T_) == ("nearest", 8)          # drawn in full on the host from --seed
