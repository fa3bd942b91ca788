"""FRePo without a GPU: the library guards every ``vdf_`` entry point (include/vd_frepo.h; its binding, layout and hashes:
tests/test_cabi.py), the float32 restatement of the header's Adam formula
(tests/frepo_oracle.py) stays within its derived bound of an fp64 Adam -- and so does torch's own CPU Adam / AdamW -- and the
host logic of frepo.py (label margin, labels, pool bookkeeping, the s2d draw) and the driver's parser follow the reference."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch

from tests import frepo_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _batch(hip, nseg, buf, n=4):
    b = hip.VdfAdamBatch()
    b.nseg = nseg
    for k in range(max(0, min(nseg, 16))):
        s = b.seg[k]
        s.p = s.m = s.v = s.g = buf
        s.n = n
    return b


def test_argument_errors_come_back_before_any_device_call():
    """No device is present here: a call that reached HIP would not return -1."""
    from video_distillation_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_float * 64)()
    a = ctypes.addressof(buf)
    for k in range(4):          # each pointer of vdf_mse_loss in turn
        args = [a, a, a, a]
        args[k] = None
        assert lib.vdf_mse_loss(args[0], args[1], 2, 2, args[2], args[3], None) == -1, k
    for B, K in ((0, 2), (2, 0), (-1, 2), (2, -3)):
        assert lib.vdf_mse_loss(a, a, B, K, a, a, None) == -1, (B, K)
    assert lib.vdf_adam_multi(None, None) == -1
    for nseg in (0, -1, 17, 1 << 20):
        assert lib.vdf_adam_multi(ctypes.addressof(_batch(hip, nseg, a)), None) == -1, nseg
    for field in ("p", "m", "v", "g"):
        for at in (0, 2):
            b = _batch(hip, 3, a)
            setattr(b.seg[at], field, None)
            assert lib.vdf_adam_multi(ctypes.addressof(b), None) == -1, (field, at)
    for n in (0, -5):
        b = _batch(hip, 2, a)
        b.seg[1].n = n
        assert lib.vdf_adam_multi(ctypes.addressof(b), None) == -1, n


def test_the_python_wrappers_refuse_on_the_host():
    from video_distillation_amd import hip, frepo
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.mse_loss(torch.zeros(2, 3), torch.zeros(2, 3))
    with pytest.raises(ValueError):
        hip.mse_loss(torch.zeros(2, 3), torch.zeros(3, 2))
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.adam_multi([(z, z, z, z, 1e-3, 0.0)], 0.9, 0.999, 1e-8, 1)
    with pytest.raises(ValueError):
        hip.adam_multi([(z, z, z, z, 1e-3, 0.0)], 0.9, 0.999, 1e-8, 0)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(NotImplementedError):
        frepo.hip_adam_step(torch.optim.Adam([p], amsgrad=True))
    with pytest.raises(NotImplementedError):
        frepo.hip_adam_step(torch.optim.SGD([p], lr=0.1))
    with pytest.raises(NotImplementedError):          # coupled (L2) weight decay is not what the kernel restates
        frepo.hip_adam_step(torch.optim.Adam([p], weight_decay=0.1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        frepo.hip_adam_step(torch.optim.Adam([p]))


# ---- the Adam restatement ------------------------------------------------------------------------
ADAM_CASES = [(t, kind, wd) for t in O.T_VALUES for kind, wd in (("randn", 0.0), ("randn", 5e-4), ("zero", 0.0), ("tiny", 0.0), ("tiny", 5e-4))]


def _torch_step(p, m, v, g, t, lr, wd):
    """One step of torch's own CPU optimiser in float32 from the state (p, m, v) before step ``t``."""
    par = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = (torch.optim.AdamW([par], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd) if wd
           else torch.optim.Adam([par], lr=lr, betas=(0.9, 0.999), eps=1e-8))
    opt.state[par] = {"step": torch.tensor(float(t - 1)), "exp_avg": torch.from_numpy(m.copy()), "exp_avg_sq": torch.from_numpy(v.copy())}
    par.grad = torch.from_numpy(g.copy())
    opt.step()
    st = opt.state[par]
    assert float(st["step"]) == t
    return par.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("t,kind,wd", ADAM_CASES)
def test_the_float32_restatement_and_torchs_adam_stay_within_the_derived_bound_of_fp64(t, kind, wd):
    """The header's formula rounds R = 12 times on the way to the quotient u -- 3 in m (difference, product, sum), 4 in v
    (product, square, product, sum), 5 in u (square root, quotient, sum, product, quotient) -- and once more in the final
    subtraction; AdamW's decay adds two roundings relative to |p|.  From one float32 state, against the fp64 step:

        |p32 - p64| <= 2^-24 |p64| [+ 2 x 2^-24 |p (1 - lr_wd)| with decay] + (R + 2) 2^-24 step_size (|m| + (1-b1)|g - m|) / denom64
        |m32 - m64| <= 3 x 2^-24 (|m| + (1-b1)|g - m|)
        |v32 - v64| <= 4 x 2^-24 v64 + 2^-149

    (tests/frepo_oracle.py ``bounds`` has the derivation).  The bound is derived, not measured; torch's own CPU Adam / AdamW in
    float32 evaluates the same update in a slightly different order (a fused lerp, addcdiv) and has to meet it too."""
    n, lr = 4096, 1e-3
    p, m, v, g = O.state(n, t, 7, kind)
    c = O.constants(lr, 0.9, 0.999, 1e-8, t, wd)
    p64, m64, v64, _, _, _ = O.adam_f64(p, m, v, g, c)
    bp, bm, bv = O.bounds(p, m, v, g, c)
    if kind == "tiny":
        assert np.all(np.abs(g) == np.float32(1e-20)) and np.all((g * g).astype(np.float32) < np.finfo(np.float32).tiny)
    for who, (p32, m32, v32) in (("restatement", O.adam_f32(p, m, v, g, c)), ("torch", _torch_step(p, m, v, g, t, lr, wd))):
        assert p32.dtype == m32.dtype == v32.dtype == np.float32
        for name, got, want, bound in (("p", p32, p64, bp), ("m", m32, m64, bm), ("v", v32, v64, bv)):
            err = np.abs(got.astype(np.float64) - want)
            worst = float(np.max(err / np.maximum(bound, 1e-300)))
            print("%s t=%d %s wd=%g: %s uses %.3f of its bound" % (who, t, kind, wd, name, worst))
            assert np.all(err <= bound), (who, name, worst)
    assert np.any(p64 != p.astype(np.float64)) or kind == "zero" and t == 1 and wd == 0


def test_the_constants_are_torchs():
    """step_size and bc2_sqrt in double, as torch.optim.Adam computes them, rounded to float once."""
    from video_distillation_amd import hip
    for t in O.T_VALUES:
        s, b = hip.adam_constants(1e-3, 0.9, 0.999, t)
        assert s == 1e-3 / (1 - 0.9 ** t) and b == (1 - 0.999 ** t) ** 0.5
        c = O.constants(1e-3, 0.9, 0.999, 1e-8, t)
        assert c["step_size"] == np.float32(s) and c["bc2_sqrt"] == np.float32(b)


# ---- the method's host logic ---------------------------------------------------------------------
def test_lb_margin_th_is_the_references_vmapped_form():
    from video_distillation_amd import frepo

    def reference_row(logits):          # distill_s2d.py:21-26, the body under @vmap
        dim = logits.shape[-1]
        val, _ = torch.topk(logits, k=2)
        return -torch.minimum(val[0] - val[1], torch.tensor(1 / dim, dtype=torch.float))

    g = torch.Generator().manual_seed(0)
    for C in (3, 10, 50):
        y = torch.randn(64, C, generator=g) * (2.0 / C)
        top = torch.topk(y, 2, dim=-1).values
        margins = top[:, 0] - top[:, 1]
        assert bool((margins > 0).all()) and bool((margins > 1 / C).any()) and bool((margins < 1 / C).any())
        want = torch.stack([reference_row(row) for row in y])
        assert torch.equal(frepo.lb_margin_th(y), want)


@pytest.mark.parametrize("C", [3, 10, 50])
def test_the_label_construction(C):
    from video_distillation_amd import frepo
    import torch.nn.functional as F
    lab = torch.arange(C).repeat_interleave(2)
    scale = np.sqrt(C / 10)
    assert frepo.y_scale(C) == float(scale)
    want_syn = (F.one_hot(lab, num_classes=C) - 1 / C) / scale          # distill_s2d.py:253, 263
    want_real = F.one_hot(lab, num_classes=C) - 1 / C          # :254-255
    assert torch.equal(frepo.soft_labels(lab, C, frepo.y_scale(C)), want_syn.float())
    assert torch.equal(frepo.soft_labels(lab, C), want_real.float())
    assert frepo.soft_labels(lab, C).dtype == torch.float32 and abs(float(frepo.soft_labels(lab, C).sum())) < 1e-4


class _StubModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(2))
        self.calls = 0

    def hip_regress_step(self, x, y, optimizer):          # a stub step: torch's own optimiser on a constant gradient
        self.calls += 1
        self.w.grad = torch.ones(2)
        optimizer.step()
        return None, None


def _stub_pool(max_updates=100, states=10, lr_net=1e-3):
    from video_distillation_amd import frepo
    return frepo.build_pool(_StubModel, lr_net, max_updates, states, "cpu")


def test_pool_bookkeeping_follows_the_reference():
    from video_distillation_amd import frepo
    pools = _stub_pool()
    assert [e.step for e in pools] == list(range(0, 100, 10))
    assert all(isinstance(e.optimizer, torch.optim.Adam) and e.optimizer.param_groups[0]["betas"] == (0.9, 0.999) for e in pools)
    assert all(e.optimizer.param_groups[0]["lr"] == pytest.approx(1e-5) for e in pools)          # (the schedule is not advanced to ``step``)
    # the learning-rate sequence equals torch's ChainedScheduler on a dummy parameter
    dummy = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1e-3, betas=(0.9, 0.999))
    S = torch.optim.lr_scheduler
    sched = S.ChainedScheduler([S.LinearLR(dummy, start_factor=0.01, total_iters=500), S.CosineAnnealingLR(dummy, T_max=100, eta_min=1e-5)])
    e = pools[7]          # starts at step 70: resets after exactly 30 steps
    x, y = torch.zeros(6, 1), torch.zeros(6, 3)
    first_model = e.model
    for k in range(29):
        assert e.optimizer.param_groups[0]["lr"] == dummy.param_groups[0]["lr"], k
        e.train_steps(x, y, steps=1)
        dummy.step(); sched.step()
        assert e.step == 71 + k and e.model is first_model and e.model.training
    assert first_model.calls == 29 and float(e.optimizer.state[e.model.w]["step"]) == 29
    e.train_steps(x, y, steps=1)          # step 100 >= max_online_updates: a fresh model, optimiser and schedule
    assert e.step == 0 and e.model is not first_model and first_model.calls == 30
    assert len(e.optimizer.state) == 0 and e.optimizer.param_groups[0]["lr"] == pytest.approx(0.01 * 1e-3)
    # get_batch: the whole set below batch_size, otherwise np.random.choice without replacement
    assert e.get_batch(x, y)[0] is x
    small = frepo.PoolElement(_StubModel, lambda m: torch.optim.Adam(m.parameters()), lambda o: frepo.chained_schedule(o, 500, 100, 1e-5),
                              torch.nn.MSELoss(), 4, 100, 0, "cpu")
    xs, ys = torch.arange(6.0)[:, None], torch.arange(6.0)[:, None].repeat(1, 3)
    np.random.seed(5)
    want = np.random.choice(6, size=(4,), replace=False)
    np.random.seed(5)
    bx, by = small.get_batch(xs, ys)
    assert bx[:, 0].tolist() == want.tolist() and by[:, 0].tolist() == want.tolist() and len(set(want.tolist())) == 4


class _StandIn(torch.nn.Module):
    """A hallucinator stand-in on CPU tensors: per clip, static (summed over its channels) + dynamic, times its own factor."""

    def __init__(self, k):
        super().__init__()
        self.k = torch.nn.Parameter(torch.tensor(float(k)))

    def forward(self, static, dynamic):
        return (static.sum(1)[:, None, None] + dynamic) * self.k


def test_s2d_syn_data_draws_and_indexes_as_the_reference_loop():
    from video_distillation_amd import frepo
    g = torch.Generator().manual_seed(1)
    n_c, dpc, T, H = 3, 2, 4, 5
    static, dynamic = torch.randn(n_c * dpc, 3, H, H, generator=g), torch.randn(n_c, dpc, T, 1, H, H, generator=g)
    hals = torch.nn.ModuleList([_StandIn(k) for k in (1, 2, 3)])
    y = torch.zeros(n_c * dpc, n_c)
    data = frepo.S2DSynData(static.clone(), dynamic.clone(), hals, y)
    for seed in (0, 1, 2):
        random.seed(seed)
        x_syn = []
        for i in range(n_c * dpc):          # distill_s2d.py:70-80
            hal_idx = random.randint(0, len(hals) - 1)
            dynamic_idx = i % dpc
            static_idx = i
            hal = hals[hal_idx]
            dyn = dynamic[i // dpc, dynamic_idx, :, :, :, :]
            sta = static[static_idx, :, :, :]
            x = hal(sta.unsqueeze(0), dyn.unsqueeze(0))
            x_syn.append(x[0])
        want, after = torch.stack(x_syn), random.random()
        random.seed(seed)
        got, y_got = data()
        assert random.random() == after          # the same number of draws, in the same order
        assert torch.equal(got.detach(), want.detach()) and y_got is data.y_syn
        random.seed(seed)
        assert torch.equal(data.value()[0], want.detach())          # value() re-draws
    got.sum().backward()
    assert data.dynamic.grad is not None and data.static.grad is None and not data.static.requires_grad
    assert not data.y_syn.requires_grad and frepo.S2DSynData(static, dynamic, hals, y, learn_label=True).y_syn.requires_grad
    one = frepo.S2DSynData(static.clone(), dynamic.clone(), torch.nn.ModuleList([_StandIn(2)]), y)          # one hallucinator: one call
    assert torch.equal(one()[0], (static.sum(1)[:, None, None] + dynamic.reshape(n_c * dpc, T, 1, H, H)) * 2)
    with pytest.raises(ValueError, match="out of range"):
        frepo.S2DSynData(static[:5], dynamic, hals, y)
    names = [n for n, _ in data.named_parameters()]
    assert [n for n in names if 'dynamic' in n] == ["dynamic"] and "static" in names and "y_syn" in names


def test_the_synthetic_optimiser_has_the_references_two_groups():
    from video_distillation_amd import frepo
    data = frepo.S2DSynData(torch.zeros(2, 3, 4, 4), torch.zeros(2, 1, 2, 1, 4, 4), torch.nn.ModuleList([_StandIn(1)]), torch.zeros(2, 2))
    opt, sch = frepo.syn_optimizer(data, 100.0, 1e-3, 50)
    assert type(opt) is torch.optim.Adam and [g["lr"] for g in opt.param_groups] == [100.0, 1e-3]
    assert opt.param_groups[0]["params"] == [data.dynamic] and len(opt.param_groups[1]["params"]) == 3
    assert isinstance(sch, torch.optim.lr_scheduler.CosineAnnealingLR) and sch.T_max == 50 and sch.eta_min == pytest.approx(1e-4)
    clips = frepo.SynData(torch.zeros(2, 2, 3, 4, 4), torch.zeros(2, 2), learn_label=True)
    opt, _ = frepo.syn_optimizer(clips, 100.0, 1e-3, 50)
    assert opt.param_groups[0]["params"] == [clips.x_syn] and opt.param_groups[1]["params"] == [clips.y_syn]


REFERENCE_DEFAULTS = dict(          # FRePo/script/distill_s2d.py:393-428, as literals
    dataset='miniUCF101', method='FRePo', model='ConvNet3D', num_prototypes_per_class=1, num_eval=5, eval_it=1000, eval_mode='S',
    epoch_eval_train=500, batch_train=None, batch_syn=512, init='real', startIt=0, Iteration=10000, max_online_updates=100,
    num_nn_state=10, learn_label=False, lr_d=1e2, lr_h=0.001, lr_net=0.001, num_workers=16, path_static=None, dpc=1, spc=1, n_hal=1,
    frames=16)


def test_parser_defaults_are_the_references():
    from video_distillation_amd import run_frepo
    args = run_frepo.build_parser().parse_args([])
    for name, want in REFERENCE_DEFAULTS.items():
        assert getattr(args, name) == want and type(getattr(args, name)) is type(want), name
    # the project's own flags; --data_path is the other drivers' relative directory, not the reference author's absolute path
    assert args.data_path == 'distill_utils/data' and args.memories == 's2d' and args.seed == 0 and args.save_path == './logged_files'
    assert args.no_eval is False and args.log_file is None and args.data_file is None and args.eval_ranks == 'rank0' and args.im_size == 112
    assert run_frepo.build_parser().parse_args(['--dataset', 'toy', '--data_file', 'f.pt', '--memories', 'images']).dataset == 'toy'
    assert (run_frepo.STEPS_PER_SAVE, run_frepo.REAL_BATCH) == (400, 512)


def test_what_the_driver_refuses(monkeypatch):
    from video_distillation_amd import run_frepo
    parse = run_frepo.build_parser().parse_args
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="single rank"):
        run_frepo.run(parse(['--dataset', 'synthetic']))
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match="eval_ranks"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--eval_ranks', 'all']))
    with pytest.raises(ValueError, match="resident"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--test_videos', 'resident']))
    with pytest.raises(ValueError, match="dpc"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--dpc', '2']))


def test_no_file_of_the_method_imports_the_oracle_or_solves_in_torch():
    for name in ("frepo.py", "run_frepo.py"):
        src = open(os.path.join(ROOT, "video_distillation_amd", name)).read()
        assert "import oracle" not in src and "from oracle" not in src and "linalg.solve" not in src and "wandb.init" not in src
