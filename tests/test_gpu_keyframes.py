"""The ``vdk_`` kernels of csrc/keyframes.hip through the C ABI against host loops of ``np.float32`` operations and against fp64,
``distill.KeyframeDMTrainer`` against the clip trainer (K = T over three steps; K = 3 at step 0) and against the oracle backend
(three steps), and ``run_dm --memories keyframes`` end to end.

Shapes: (5, 7) has 3*H*W = 105, no multiple of 4: the scalar kernels; (6, 6) = 27 float4, less than one workgroup of the vector
kernels, whose bound check cuts the block; (64, 64) = 3072 float4 = 12 workgroups per frame; the same (6, 6) from a base 4 bytes
off a 16-byte boundary takes the scalar kernels again.  Tables (T, K): (1,1), (8,1), (5,2), (8,3), (16,4), (16,16) linear and
(8,3), (16,4) nearest; n = 1, 3.  32 770 clips of (2, 2) with T = K = 2 are 65 540 (clip, key) pairs: grid y is capped at
65 535, so reduce's pair loop takes a second turn.

Tolerances.  Both kernels compute stated fp32 operations in a stated order: compared bit for bit with the host loops
(tests/test_keyframes_cpu.py ``np_expand`` / ``np_reduce``), and a second run with the first.  Against fp64 with the fp32 table
weights: expand is two products and one add, each within 2^-24 relative of its own result, which is at most
|w0 k0| + |w1 k1|: 3 * 2^-24 * (|w0 k0| + |w1 k1|); reduce for a key with m terms is m products and m - 1 adds, every partial sum
at most sum |w g|: 2 m * 2^-24 * sum |w g|.  Trainer against the oracle: the project's bars (loss 1e-3 relative,
tests/test_gpu_e2e.py; memory update 5e-2 rel-l2 per class, tests/test_gpu_still.py); tests/test_keyframes_cpu.py asserts the
fp32 oracle ten times inside both against float64."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
SHAPES = [(5, 7), (6, 6), (64, 64)]


def _call(name, *args):
    from video_distillation_amd import hip
    rc = getattr(hip.lib(), name)(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _guarded(numel, offset=0):
    """A device buffer of ``numel`` floats starting ``offset`` floats into an allocation, NaN-filled, with ``GUARD`` floats of a
    sentinel behind it -> (the allocation, the view to hand to the kernel)."""
    whole = torch.full((offset + numel + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    whole[offset + numel:] = -777.0
    return whole, whole[offset:offset + numel]


def _guard_intact(whole, numel, offset=0):
    return bool((whole[offset + numel:] == -777.0).all()) and (offset == 0 or bool(torch.isnan(whole[:offset]).all()))


def _device(a, offset=0):
    whole = torch.zeros(offset + a.size, dtype=torch.float32, device="cuda")
    src = whole[offset:]
    src.copy_(torch.from_numpy(a).reshape(-1))
    assert (src.data_ptr() % 16 == 0) == (offset == 0)
    return whole, src


def _data(rng, shape):
    """Normal values with a magnitude per frame spread over six decades."""
    return (rng.normal(0.0, 1.0, shape) * 10.0 ** rng.integers(-3, 3, shape[:2] + (1, 1, 1))).astype(np.float32)


def _run_twice(name, src, n, tab, H, W, out_numel, offset):
    from video_distillation_amd import hip
    ctab = hip.vdk_table(tab)
    outs = []
    for _ in range(2):
        whole, out = _guarded(out_numel, offset)
        assert (out.data_ptr() % 16 == 0) == (offset == 0)
        assert _call(name, src.data_ptr(), n, ctypes.addressof(ctab), H, W, out.data_ptr()) == 0
        assert _guard_intact(whole, out_numel, offset)
        outs.append(out.cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))          # a second run: identical bits
    return outs[0]


def _expand_case(n, T, K, interp, H, W, offset=0):
    from tests.test_keyframes_cpu import np_expand
    from video_distillation_amd import keyframes
    tab = keyframes.table(T, K, interp)
    keys = _data(np.random.default_rng(1000 * H + 10 * T + K + n), (n, K, 3, H, W))
    keep, src = _device(keys, offset)
    got = _run_twice("vdk_keyframe_expand", src, n, tab, H, W, n * T * 3 * H * W, offset).reshape(n, T, 3, H, W)
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), np_expand(keys, tab).view(np.uint32))
    k64 = keys.astype(np.float64)
    for t in range(T):
        a, b = float(tab.w0[t]) * k64[:, tab.i0[t]], float(tab.w1[t]) * k64[:, tab.i1[t]]
        assert (np.abs(got[:, t].astype(np.float64) - (a + b)) <= 3 * 2.0 ** -24 * (np.abs(a) + np.abs(b))).all(), t
    if K == T:
        assert np.array_equal(got.view(np.uint32), keys.view(np.uint32))          # a copy
    if K == 1:          # the still clip, bit for bit
        whole, out = _guarded(n * T * 3 * H * W, offset)
        assert _call("vds_still_expand", src.data_ptr(), 0, n, T, H, W, out.data_ptr()) == 0
        assert np.array_equal(out.cpu().numpy().view(np.uint32), got.reshape(-1).view(np.uint32))


def _reduce_case(n, T, K, interp, H, W, offset=0):
    from tests.test_keyframes_cpu import np_reduce
    from video_distillation_amd import keyframes
    tab = keyframes.table(T, K, interp)
    g = _data(np.random.default_rng(2000 * H + 10 * T + K + n), (n, T, 3, H, W))
    keep, src = _device(g, offset)
    got = _run_twice("vdk_keyframe_reduce", src, n, tab, H, W, n * K * 3 * H * W, offset).reshape(n, K, 3, H, W)
    assert not np.isnan(got).any()
    assert np.array_equal(got.view(np.uint32), np_reduce(g, tab).view(np.uint32))
    g64 = g.astype(np.float64)
    for k in range(K):
        terms = tab.terms(k)
        exact = sum(w * g64[:, t] for t, w in terms)
        mag = sum(abs(w) * np.abs(g64[:, t]) for t, w in terms)
        assert len(terms) >= 1 and (np.abs(got[:, k].astype(np.float64) - exact) <= 2 * len(terms) * 2.0 ** -24 * mag).all(), k
    if K == T:
        assert np.array_equal(got.view(np.uint32), g.view(np.uint32))
    if K == 1:
        whole, out = _guarded(n * 3 * H * W, offset)
        assert _call("vds_still_reduce", src.data_ptr(), n, T, H, W, out.data_ptr()) == 0
        assert np.array_equal(out.cpu().numpy().view(np.uint32), got.reshape(-1).view(np.uint32))


def _tables():
    from tests.test_keyframes_cpu import TABLES
    return TABLES


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("T,K,interp", _tables())
def test_expand_and_reduce_are_the_float32_host_loops_bit_for_bit(T, K, interp, H, W):
    for n in (1, 3):
        _expand_case(n, T, K, interp, H, W)
        _reduce_case(n, T, K, interp, H, W)


@pytest.mark.parametrize("T,K,interp", _tables())
def test_bases_off_a_16_byte_boundary_take_the_scalar_kernels(T, K, interp):
    _expand_case(3, T, K, interp, 6, 6, offset=1)
    _reduce_case(3, T, K, interp, 6, 6, offset=1)


def test_more_pairs_than_one_pass_of_the_grid():
    n = 32770
    assert n * 2 > 65535
    _expand_case(n, 2, 2, "linear", 2, 2)
    _reduce_case(n, 2, 2, "linear", 2, 2)
    _reduce_case(n, 2, 2, "nearest", 2, 2)


def test_an_empty_batch_writes_nothing_and_a_zero_weight_never_meets_an_infinity():
    from video_distillation_amd import hip, keyframes
    tab = keyframes.table(8, 3)
    ctab = hip.vdk_table(tab)
    whole, out = _guarded(32)
    x = torch.randn(1, 3, 3, 6, 6).cuda()
    assert _call("vdk_keyframe_expand", x.data_ptr(), 0, ctypes.addressof(ctab), 6, 6, out.data_ptr()) == 0
    assert _call("vdk_keyframe_reduce", x.data_ptr(), 0, ctypes.addressof(ctab), 6, 6, out.data_ptr()) == 0
    assert bool(torch.isnan(whole[:32]).all()) and _guard_intact(whole, 32)
    # key 2 is all infinities: frames 0..3 do not use it (weight 0 at t = 0 of a segment, other keys elsewhere) and stay finite
    keys = torch.randn(2, 3, 3, 6, 6)
    keys[:, 2] = float("inf")
    got = hip.keyframe_expand(keys.cuda(), tab).cpu()
    uses = [t for t in range(8) if 2 in [int(i) for i, w in ((tab.i0[t], tab.w0[t]), (tab.i1[t], tab.w1[t])) if w != 0]]
    assert uses == [4, 5, 6, 7] and bool(torch.isfinite(got[:, :4]).all()) and bool(torch.isinf(got[:, 4:]).all())
    g = torch.randn(2, 8, 3, 6, 6)
    g[:, 7] = float("inf")          # the last frame belongs to the last key alone (w0 = 0 there)
    back = hip.keyframe_reduce(g.cuda(), tab).cpu()
    assert bool(torch.isfinite(back[:, :2]).all()) and bool(torch.isinf(back[:, 2]).all())


def test_python_wrappers_validate_on_the_host():
    from video_distillation_amd import hip, keyframes
    tab = keyframes.table(8, 3)
    keys = torch.randn(2, 3, 3, 5, 7).cuda()
    out = hip.keyframe_expand(keys, tab)
    assert out.shape == (2, 8, 3, 5, 7) and torch.equal(out[:, 0], keys[:, 0]) and torch.equal(out[:, 7], keys[:, 2])
    assert hip.keyframe_reduce(out, tab).shape == (2, 3, 3, 5, 7)
    with pytest.raises(ValueError):
        hip.keyframe_expand(torch.randn(2, 4, 3, 5, 7).cuda(), tab)
    with pytest.raises(ValueError):
        hip.keyframe_reduce(keys, tab)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.keyframe_expand(keys.transpose(3, 4), tab)
    assert hip.keyframe_expand(keys[:0], tab).shape == (0, 8, 3, 5, 7)


# ---- trainer --------------------------------------------------------------------------------------------------------------

class _OracleNets:
    """A backend whose fresh network of iteration ``it`` is the oracle's of seed ``it``, as ``OracleBackend.new_network`` gives."""

    def __init__(self, inner):
        self.inner = inner

    def __getattr__(self, k):
        return getattr(self.inner, k)

    def new_network(self, seed):
        from oracle import ref_cpu as R
        return [p.cuda() for p in R.init_params(int(seed))[:6]]


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _hip_backend(**kw):
    from tests.test_keyframes_cpu import HW, T
    from video_distillation_amd import distill, plan
    return _OracleNets(distill.HipBackend(plan.NetGeometry(T, HW, HW), "cuda:0", **kw))


def _clip_trainer(clips, image_syn, batch_real, steps):
    """``DMTrainer`` on the HIP backend from ``image_syn`` -> (losses, image_syn, buf) on the host."""
    from tests.test_keyframes_cpu import C, IPC, LR, MU, PER
    from video_distillation_amd import distill
    pool = distill.RealPool(clips, [PER] * C, [c * PER for c in range(C)])
    tr = distill.DMTrainer(_hip_backend(), pool, C, IPC, batch_real, LR, momentum=MU, image_syn=image_syn.clone())
    losses = [float(tr.step(it)) for it in range(steps)]
    torch.cuda.synchronize()
    return losses, tr.image_syn.cpu().clone(), tr.buf.cpu().clone()


def _keyframe_trainer(clips, K, interp, batch_real):
    from tests.test_keyframes_cpu import C, IPC, LR, MU, PER
    from tests.test_keyframes_cpu import T, HW
    from video_distillation_amd import distill, plan
    pool = distill.RealPool(clips, [PER] * C, [c * PER for c in range(C)])
    return distill.KeyframeDMTrainer(_hip_backend(), pool, plan.NetGeometry(T, HW, HW), C, IPC, batch_real, LR, key_frames=K,
                                     interp=interp, momentum=MU)


def test_k_equal_t_is_the_clip_trainer_over_three_steps():
    """K = T: expand and reduce are copies, so every launch of a step is the clip trainer's on the same bytes.  The bar is the
    clip trainer's own run-to-run distance, measured here and expected to be zero (no launch of a DM step accumulates with
    atomics): losses and memories then agree bit for bit.  Were it not zero, the bar would be four times that distance."""
    from tests.test_keyframes_cpu import BATCH, PER, STEPS, T, keyframe_case
    clips = keyframe_case().cuda()
    syn0 = clips[[0, 1, PER, PER + 1]].clone()
    la, xa, _ = _clip_trainer(clips, syn0, BATCH, STEPS)
    lb, xb, _ = _clip_trainer(clips, syn0, BATCH, STEPS)
    tr = _keyframe_trainer(clips, T, "linear", BATCH)
    assert torch.equal(tr.keys, syn0)
    lk = [float(tr.step(it)) for it in range(STEPS)]
    torch.cuda.synchronize()
    d_loss, d_x = max(abs(a - b) for a, b in zip(la, lb)), _rel(xa, xb)
    print("K = T, %d steps: clip trainer twice: losses %s / %s, memories rel-l2 %.3e; key-frame trainer: losses %s, memories rel-l2 %.3e"
          % (STEPS, la, lb, d_x, lk, _rel(tr.keys.cpu(), xa)))
    assert not torch.equal(xa, syn0.cpu()) and torch.equal(tr.image_syn, tr.keys)
    if d_loss == 0 and d_x == 0:
        assert lk == la and torch.equal(tr.keys.cpu(), xa)
    else:
        assert max(abs(a - b) for a, b in zip(lk, la)) <= 4 * d_loss and _rel(tr.keys.cpu(), xa) <= 4 * d_x


@pytest.mark.parametrize("batch_real", [8, 2])
def test_step_0_at_k_3_equals_the_clip_trainer_on_the_expanded_keys(batch_real):
    """K = 3 linear against ``DMTrainer`` with ``image_syn = expand(keys)``: the same launches on the same bytes up to the pixel
    gradient, so the loss is the clip trainer's and the first step's ``buf`` -- the gradient itself -- is
    ``keyframe_reduce(clip trainer's buf)``, bit for bit under the rule of the test above (the clip trainer's own run-to-run
    distance, expected zero, else four times it).  batch_real 8 deals the real clips to dither sets, 2 takes the plain forward."""
    from tests.test_keyframes_cpu import keyframe_case
    from video_distillation_amd import hip
    clips = keyframe_case().cuda()
    tr = _keyframe_trainer(clips, 3, "linear", batch_real)
    syn0 = tr.image_syn.clone()
    assert torch.equal(syn0, hip.keyframe_expand(tr.keys, tr.table)) and torch.equal(syn0[:, 0], clips[[0, 1, 12, 13]][:, 0])
    (la,), _, ba = _clip_trainer(clips, syn0, batch_real, 1)
    (lb,), _, bb = _clip_trainer(clips, syn0, batch_real, 1)
    ga, gb = hip.keyframe_reduce(ba.cuda(), tr.table).cpu(), hip.keyframe_reduce(bb.cuda(), tr.table).cpu()
    lk = float(tr.step(0))
    torch.cuda.synchronize()
    d_loss, d_g = abs(la - lb), _rel(ga, gb)
    print("step 0, K 3, batch_real %d: clip trainer twice: loss %.9g / %.9g, reduced gradient rel-l2 %.3e; key-frame trainer: loss %.9g, "
          "buf rel-l2 to the reduced clip gradient %.3e" % (batch_real, la, lb, d_g, lk, _rel(tr.buf.cpu(), ga)))
    assert float(ga.abs().max()) > 0 and np.isfinite(lk)
    if d_loss == 0 and d_g == 0:
        assert lk == la and torch.equal(tr.buf.cpu(), ga)
    else:
        assert abs(lk - la) <= 4 * d_loss and _rel(tr.buf.cpu(), ga) <= 4 * d_g


def _hip_steps(clips, K, interp, overlap):
    from tests.test_keyframes_cpu import BATCH, STEPS
    from video_distillation_amd import hip
    tr = _keyframe_trainer(clips, K, interp, BATCH)
    losses = [tr.step(it, overlap=overlap) for it in range(STEPS)]
    tr.sync()
    torch.cuda.synchronize()
    assert torch.equal(tr.image_syn, hip.keyframe_expand(tr.keys, tr.table))
    return [float(v) for v in losses], tr.keys.cpu().clone()


@pytest.mark.parametrize("K,interp", [(3, "linear"), (2, "nearest")])
def test_three_steps_match_the_oracle_with_and_without_overlap(K, interp):
    """HIP (the shipped mixed mode) against ``OracleBackend`` on the inputs of tests/test_keyframes_cpu.py: loss within 1e-3
    relative at every step, key update (keys after three steps - keys before) within 5e-2 rel-l2 per class, arg-max flips
    allowed.  K = 2 nearest has four equal frames per key: the temporal max-pool meets exact ties between them, and which of two
    equal frames takes the gradient does not change the sum over a key's frames (distill.StillGMTrainer's argument) -- this case
    tests that.  ``overlap=True`` must give the same keys and losses as without, bit for bit: two plain runs agree bit for bit
    (asserted first), and overlap changes when a launch is issued, not what it computes."""
    from tests.test_keyframes_cpu import C, IPC, oracle_steps
    want = oracle_steps(K, interp)
    clips, keys0 = want["clips"].cuda(), want["keys0"]
    l_plain, k_plain = _hip_steps(clips, K, interp, False)
    l_again, k_again = _hip_steps(clips, K, interp, False)
    l_over, k_over = _hip_steps(clips, K, interp, True)
    for name, losses, keys in (("plain", l_plain, k_plain), ("overlap", l_over, k_over)):
        rel_loss = [abs(a - b) / b for a, b in zip(losses, want["losses"])]
        per = [_rel(keys[c * IPC:(c + 1) * IPC] - keys0[c * IPC:(c + 1) * IPC],
                    want["keys"][c * IPC:(c + 1) * IPC] - keys0[c * IPC:(c + 1) * IPC]) for c in range(C)]
        print("key-frame DM, K %d %s, 3 steps, %s: loss rel %s; key update rel-l2 per class %s"
              % (K, interp, name, ["%.1e" % e for e in rel_loss], ["%.1e" % e for e in per]))
        assert max(rel_loss) < 1e-3 and max(per) < 5e-2, name
    d = _rel(k_again, k_plain)
    print("two plain runs: rel-l2 %.3e; overlap against plain: %.3e" % (d, _rel(k_over, k_plain)))
    assert d == 0 and torch.equal(k_again, k_plain) and l_again == l_plain
    assert torch.equal(k_over, k_plain) and l_over == l_plain


def test_run_dm_keyframes_end_to_end(tmp_path):
    """``run_dm --memories keyframes`` on the HIP backend: toy data with test clips, 2 classes, Iteration 1, one evaluation of
    one epoch at iteration 0.  The file of iteration 0 holds the ``--init real`` keys; expanded on the host
    (``checkpoint.keyframes_to_images``) it equals the device expansion bit for bit, and so does the trainer's final state."""
    from video_distillation_amd import checkpoint, distill, hip, keyframes, run_dm
    Cn, per, Tn, S = 2, 4, 8, 64
    g = torch.Generator().manual_seed(8)
    clips, labels = torch.randn(Cn * per, Tn, 3, S, S, generator=g), torch.arange(Cn).repeat_interleave(per)
    test_clips, test_labels = torch.randn(8, Tn, 3, S, S, generator=g), torch.arange(8) % Cn
    torch.save({"clips": clips, "labels": labels, "test_clips": test_clips, "test_labels": test_labels}, tmp_path / "toy.pt")
    args = run_dm.build_parser().parse_args([
        "--memories", "keyframes", "--key_frames", "3", "--interp", "linear", "--dataset", "toy", "--data_file", str(tmp_path / "toy.pt"),
        "--frames", str(Tn), "--im_size", str(S), "--ipc", "1", "--batch_real", "2", "--Iteration", "1", "--eval_it", "2", "--num_eval", "1",
        "--epoch_eval_train", "1", "--lr_img", "0.01", "--lr_net", "0.01", "--batch_train", "4", "--save_path", str(tmp_path / "out")])
    log = []
    tr = run_dm.run(args, log=log)
    torch.cuda.synchronize()
    assert type(tr) is distill.KeyframeDMTrainer and tr.steps_done == 2
    losses = [r["Loss"] for r in log if "Loss" in r]
    accs = [r for r in log if "Accuracy/ConvNet3D" in r]
    assert len(losses) == 2 and all(np.isfinite(losses)) and len(accs) == 1 and 0.0 <= accs[0]["Accuracy/ConvNet3D"] <= 1.0
    path = os.path.join(tmp_path, "out", "Keyframes_DM", "toy_ipc1_k3_linear_0.01", "keyframes_0.pt")
    frames, interp, T_ = checkpoint.load_keyframes(path)
    assert frames.shape == (2, 3, 3, S, S) and (interp, T_) == ("linear", Tn)
    assert torch.equal(frames, clips[[0, per]][:, [0, 4, 7]]) and not torch.equal(tr.keys.cpu(), frames)
    images = checkpoint.keyframes_to_images(path)
    assert torch.equal(images, hip.keyframe_expand(frames.cuda(), keyframes.table(Tn, 3, "linear")).cpu())
    after = checkpoint.save_keyframes(str(tmp_path / "after"), 1, tr.gather_keys(), tr.interp, Tn)
    assert torch.equal(checkpoint.keyframes_to_images(after), tr.gather_syn().cpu()) and bool(torch.isfinite(tr.keys).all())
