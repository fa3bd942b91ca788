"""run_frepo's real batches from HBM, its leader / embedder protocol and its dealt evaluation, without a GPU: the index stream is
the DataLoader's, the slices partition a batch and pad-and-trim restores it, the one name of include/vd_regress.h is guarded (its
binding and hashes: tests/test_cabi.py), the default recipe of ``evaluate_pool`` deals the units as before, the driver refuses
what it cannot run, and at one rank the protocol is a no-op around ``FRePoTrainer.step``."""
import ctypes
import inspect
import random

import numpy as np
import pytest
import torch


# ---- the index stream ----------------------------------------------------------------------------
@pytest.mark.parametrize("n,batch", [(8, 3), (6, 512), (7, 7)])
def test_real_batch_indices_are_the_dataloaders(n, batch):
    from video_distillation_amd import frepo
    g = torch.Generator().manual_seed(5)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.arange(n)), batch_size=batch, shuffle=True, generator=g)
    per_epoch = -(-n // batch)
    want = [b[0].tolist() for _ in range(4) for b in loader][:3 * per_epoch + 1]          # three epochs and the start of a fourth
    stream = frepo.real_batch_indices(n, batch, torch.Generator().manual_seed(5))
    got = [next(stream) for _ in range(len(want))]
    assert all(t.dtype == torch.int64 and t.dim() == 1 and not t.is_cuda for t in got)
    assert [t.tolist() for t in got] == want
    assert len(want[per_epoch - 1]) == n - (per_epoch - 1) * batch          # the last batch of an epoch is short
    for e in range(3):
        assert sorted(sum(want[e * per_epoch:(e + 1) * per_epoch], [])) == list(range(n))
    with pytest.raises(ValueError):
        next(frepo.real_batch_indices(0, 4, g))


# ---- slices, pad and trim ------------------------------------------------------------------------
def test_slices_partition_a_batch_and_pad_and_trim_restores_it():
    from video_distillation_amd import frepo
    for world in range(1, 5):
        for m in range(0, 10):
            cuts = [frepo.rank_slice(m, r, world) for r in range(world)]
            assert cuts[0][0] == 0 and cuts[-1][1] == m
            assert all(a[1] == b[0] for a, b in zip(cuts, cuts[1:])) and all(lo <= hi for lo, hi in cuts)
            pad = frepo.pad_rows(m, world)
            assert pad == -(-m // world) and all(hi - lo <= pad for lo, hi in cuts)
            assert max(hi - lo for lo, hi in cuts) - min(hi - lo for lo, hi in cuts) <= 1
            rows = torch.arange(m * 3, dtype=torch.float32).reshape(m, 3) + 1
            gathered = torch.full((world * pad, 3), -7.0)          # what all_gather_into_tensor leaves: rank r's buffer at r * pad
            for r, (lo, hi) in enumerate(cuts):
                gathered[r * pad:r * pad + (hi - lo)] = rows[lo:hi]
            assert torch.equal(frepo.trim_gathered(gathered, m, world), rows)
    assert frepo.rank_slice(2, 0, 3) == (0, 0) and frepo.rank_slice(8, 1, 3) == (2, 5)          # an empty slice; 2 / 3 / 3


def test_argument_errors_come_back_before_any_device_call():
    """No device is present here: a call that reached HIP would not return -1, and B == 0 would not return 0."""
    from video_distillation_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    for k in range(3):
        args = [a, a, a]
        args[k] = None
        assert lib.vdr_regress_stats(args[0], args[1], 2, 2, args[2], None) == -1, k
    for B, K in ((-1, 2), (2, 0), (2, -3), (0, 0)):
        assert lib.vdr_regress_stats(a, a, B, K, a, None) == -1, (B, K)
    assert lib.vdr_regress_stats(None, None, 0, 3, None, None) == 0          # B == 0 touches nothing
    assert all(v == 0.0 for v in buf)


def test_the_host_definitions_of_regress_stats_follow_the_header():
    """CPU tensors take the record's definitions in torch fp64 (so evalpool's host logic runs under gloo without a GPU): slot by
    slot on a batch with a tie, a label out of range on either side, and soft labels that are frepo.soft_labels' fp32 values."""
    from video_distillation_amd import frepo, hip
    K = 4
    z = torch.tensor([[0.5, 0.5, 0.1, 0.0], [0.5, 0.5, 0.1, 0.0], [1.0, 2.0, 3.0, 4.0], [0.0, 0.0, 0.0, 0.0], [9.0, 0.0, 0.0, 0.0]])
    y = torch.tensor([1, 0, 0, -1, K])
    rec = hip.regress_stats(z, y, hip.eval_stats_record(K))
    soft = frepo.soft_labels(y[:3], K).double()
    assert rec[0] == 3 and rec[5] == 2 and rec[6] == 0 and rec[7] == 0
    assert float(rec[1]) == pytest.approx(float(((z[:3].double() - soft) ** 2).sum()), rel=1e-15)
    assert rec[2:5].tolist() == [1.0, 2.0, 3.0]          # ranks 1 (tie at a lower index), 0, 3
    assert rec[8:8 + K].tolist() == [1.0, 0.0, 0.0, 0.0] and rec[8 + K:].tolist() == [2.0, 1.0, 0.0, 0.0]
    again = hip.regress_stats(z, y, rec.clone())
    assert torch.equal(again, 2 * rec)          # it accumulates
    assert torch.equal(hip.regress_stats(z[:0], y[:0], rec.clone()), rec)
    with pytest.raises(ValueError):
        hip.regress_stats(z, frepo.soft_labels(y[:3], K), rec)          # soft labels are not what it takes
    inv = np.float32(1.0 / K)
    assert frepo.soft_labels(torch.tensor([2]), K)[0].tolist() == [float(np.float32(0) - inv)] * 2 + [float(np.float32(1) - inv), float(np.float32(0) - inv)]


# ---- the recipe ----------------------------------------------------------------------------------
def test_the_default_recipe_deals_the_units_as_before():
    from video_distillation_amd import evalpool, frepo
    default = evalpool.default_recipe()
    assert default.passes == evalpool.PASSES == 3 and default.data is None and default.test_pass is evalpool.test_pass
    assert "recipe" in inspect.signature(evalpool.evaluate_pool).parameters
    assert inspect.signature(evalpool.evaluate_pool).parameters["recipe"].default is None
    for num_eval in range(1, 6):
        for world in range(1, 5):
            today = {"train": [i % world for i in range(num_eval)],
                     "test": [[(i + p * num_eval) % world for p in range(3)] for i in range(num_eval)]}
            assert evalpool.assignment(num_eval, world) == today == evalpool.assignment(num_eval, world, default.passes)
            one = evalpool.assignment(num_eval, world, 1)
            assert one["train"] == today["train"] and one["test"] == [[r] for r in today["train"]]          # one unit, one rank: the owner
            assert all(evalpool.unit_rank(i, 0, num_eval, world, 1) == evalpool.train_rank(i, world) for i in range(num_eval))
    with pytest.raises(ValueError):
        evalpool.unit_rank(0, 1, 2, 2, passes=1)
    assert frepo.EVAL_RECIPE.passes == 1 and frepo.EVAL_RECIPE.loss_scale(50) == 50.0
    other = frepo.EVAL_RECIPE.with_data(lambda i: i)
    assert other.data(3) == 3 and frepo.EVAL_RECIPE.data is None and other.train is frepo.EVAL_RECIPE.train


def test_derive_with_one_pass_reads_the_regression_record():
    from video_distillation_amd import evalpool
    K = 3
    R = torch.zeros(2, 2, 8 + 2 * K, dtype=torch.float64)
    for i, (clips, sq, hits) in enumerate(((4.0, 6.0, 3.0), (4.0, 1.5, 1.0))):
        R[i, 0, 0], R[i, 0, 1], R[i, 0, 2] = clips, sq, hits
        R[i, 0, 8 + K:] = torch.tensor([2.0, 2.0, 0.0])
        R[i, 1, 0], R[i, 1, 1] = 0.25, 0.5
    out = evalpool.derive(R, 2, 2, passes=1, loss_scale=float(K))
    assert out["acc_test"] == [0.75, 0.25] and out["loss_test"] == [6.0 / 4 / K, 1.5 / 4 / K] and out["mean"] == 0.5
    assert out["loss_train"] == [0.25, 0.25] and out["acc_train"] == [0.5, 0.5] and out["acc_per_class"][0][2] is None
    assert out["assignment"]["test"] == [[0], [1]]
    with pytest.raises(ValueError):
        evalpool.derive(R, 2, 2)          # three passes need four rows


# ---- what the driver refuses ---------------------------------------------------------------------
def test_what_the_driver_refuses_of_the_new_flags(monkeypatch):
    from video_distillation_amd import run_frepo
    parse = run_frepo.build_parser().parse_args
    args = parse([])
    assert (args.train_videos, args.target_ranks, args.eval_ranks, args.test_videos) == ('host', 'rank0', 'rank0', 'host')
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match=r"single rank.*--target_ranks all"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--train_videos', 'preload']))
    with pytest.raises(ValueError, match=r"target_ranks all needs --train_videos preload or resident"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--target_ranks', 'all']))
    with pytest.raises(ValueError, match="resident"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--train_videos', 'resident', '--target_ranks', 'all']))
    monkeypatch.setenv("WORLD_SIZE", "1")
    with pytest.raises(ValueError, match=r"eval_ranks all needs --target_ranks all"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--train_videos', 'preload', '--eval_ranks', 'all']))
    with pytest.raises(ValueError, match="resident"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--train_videos', 'resident']))
    with pytest.raises(ValueError, match="resident"):
        run_frepo.run(parse(['--dataset', 'toy', '--data_file', 'f.pt', '--train_videos', 'resident']))
    with pytest.raises(ValueError, match=r"eval_ranks all at WORLD_SIZE 1"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--train_videos', 'preload', '--target_ranks', 'all', '--eval_ranks', 'all']))
    with pytest.raises(ValueError, match="target_ranks all needs"):
        run_frepo.run(parse(['--dataset', 'synthetic', '--target_ranks', 'all']))


# ---- the protocol at one rank --------------------------------------------------------------------
class _StubNet(torch.nn.Module):
    """A CPU stand-in for ConvNet3D: a linear embedding of the flattened clip, a linear head, and the train step of
    tests/test_frepo_cpu.py's stub (torch's own optimiser on a constant gradient)."""

    def __init__(self, pixels, d, classes):
        super().__init__()
        self.features = torch.nn.Linear(pixels, d)
        self.logit = torch.nn.Linear(d, classes)
        self.exact_calls = 0

    def embed(self, x):
        return torch.tanh(self.features(x.reshape(x.shape[0], -1)))

    def embed_exact(self, x):
        self.exact_calls += 1
        with torch.no_grad():
            return self.embed(x.detach())

    def hip_regress_step(self, x, y, optimizer):
        for p in self.parameters():
            p.grad = torch.ones_like(p)
        optimizer.step()
        return None, None


def _ridge(feat_syn, y_syn, feat_tar, reg):
    """The predictor of include/vd_nfr.h in torch fp64 (a stand-in for the HIP op, which has no CPU path)."""
    fs, ft = feat_syn.double(), feat_tar.double()
    kss = fs @ fs.t()
    lam = abs(reg) * torch.trace(kss) / kss.shape[0]
    return (ft @ fs.t() @ torch.linalg.solve(kss + lam * torch.eye(kss.shape[0], dtype=torch.float64), y_syn.double())).float()


def _stub_trainer(monkeypatch):
    from video_distillation_amd import frepo, nfr
    monkeypatch.setattr(nfr, "nfr_pred", _ridge)
    monkeypatch.setattr(frepo, "hip_adam_step", lambda opt: opt.step())
    C, T, S, d = 3, 2, 4, 5
    g = torch.Generator().manual_seed(0)
    syn = frepo.SynData(torch.randn(2 * C, T, 3, S, S, generator=g),
                        frepo.soft_labels(torch.arange(C).repeat_interleave(2), C, frepo.y_scale(C)), learn_label=True)
    opt, sch = frepo.syn_optimizer(syn, 1e-2, 1e-3, 10)

    def get_model():
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(11)
            return _StubNet(T * 3 * S * S, d, C)
    pools = frepo.build_pool(get_model, 1e-3, 100, 2, "cpu")
    real = torch.randn(8, T, 3, S, S, generator=g)
    labels = torch.arange(8) % C
    return frepo.FRePoTrainer(syn, pools, opt, sch), real, labels, C


def _run(monkeypatch, protocol: bool):
    from video_distillation_amd import frepo
    trainer, real, labels, C = _stub_trainer(monkeypatch)
    random.seed(1); np.random.seed(1); torch.manual_seed(1)
    stream = frepo.real_batch_indices(8, 3, torch.Generator().manual_seed(2))
    exchange = frepo.TargetExchange(lambda idx: trainer.pools[idx].model, lambda rows: real.index_select(0, rows.reshape(-1)), 0, 1,
                                    "cpu", batch=3, width=1)
    exchange.sync_all_weights(len(trainer.pools))          # a no-op at one rank
    losses = []
    for it in range(4):          # the third batch of an epoch of 8 is short (2 clips)
        rows = next(stream).reshape(-1, 1)
        y = frepo.soft_labels(labels[rows[:, 0]], C)
        if protocol:
            idx = trainer.draw_pool_index()
            out = exchange.lead(idx, rows, lambda feat: trainer.step(None, y, feat_tar=feat, idx=idx), it)
        else:
            out = trainer.step(real.index_select(0, rows[:, 0]), y)
        losses.append([float(v) for v in out])
    if protocol:
        exchange.lead_stop()
        exchange.lead_abort()          # nothing is waiting: no second message
    state = [p.detach().clone() for p in trainer.syndata.parameters()]
    weights = [torch.cat([p.detach().reshape(-1) for p in e.model.parameters()]) for e in trainer.pools]
    return losses, state, weights, np.random.randint(1 << 30), random.random()


def test_at_one_rank_the_protocol_is_a_no_op(monkeypatch):
    plain = _run(monkeypatch, protocol=False)
    led = _run(monkeypatch, protocol=True)
    assert plain[0] == led[0] and all(np.isfinite(v) for row in plain[0] for v in row)
    assert all(torch.equal(a, b) for a, b in zip(plain[1], led[1])) and all(torch.equal(a, b) for a, b in zip(plain[2], led[2]))
    assert plain[3:] == led[3:]          # the global generators were consumed alike
    assert plain[0][0] != plain[0][1]


def test_step_with_features_needs_the_index_they_came_from(monkeypatch):
    trainer, real, labels, C = _stub_trainer(monkeypatch)
    from video_distillation_amd import frepo
    with pytest.raises(ValueError, match="idx"):
        trainer.step(None, frepo.soft_labels(labels, C), feat_tar=torch.zeros(8, 5))
    assert "feat_tar" in inspect.signature(frepo.PoolElement.nfr).parameters
    from video_distillation_amd import nfr
    assert inspect.signature(nfr.nfr).parameters["feat_tar"].default is None


def test_a_failing_step_or_embed_is_raised_after_the_exchange(monkeypatch):
    from video_distillation_amd import frepo
    trainer, real, labels, C = _stub_trainer(monkeypatch)
    exchange = frepo.TargetExchange(lambda idx: trainer.pools[idx].model, lambda rows: real.index_select(0, rows.reshape(-1)), 0, 1,
                                    "cpu", batch=3, width=1)
    rows = torch.tensor([[0], [1]])

    def bad_step(feat):
        raise KeyError("step")
    with pytest.raises(KeyError):
        exchange.lead(0, rows, bad_step)

    def inject(rank, calls):
        raise OSError("embed")
    exchange.inject = inject
    with pytest.raises(OSError):
        exchange.lead(0, rows, lambda feat: None)
    with pytest.raises(ValueError):
        frepo.TargetExchange(lambda idx: None, None, 0, 1, "cpu", batch=3).lead(0, torch.zeros(4, 1, dtype=torch.int64), None)
