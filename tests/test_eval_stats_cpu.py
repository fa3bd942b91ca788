"""hip.eval_stats on CPU tensors (the torch fp64 branch the host logic of evalpool.py runs on under gloo) against the numpy
restatement of the record's definitions (tests/eval_stats_oracle.py): counts exactly, the cross-entropy sum within 1e-12."""
import numpy as np
import pytest
import torch

from tests import eval_stats_oracle as O


def _run(z, y, rec=None):
    from video_distillation_amd import hip
    rec = hip.eval_stats_record(z.shape[1]) if rec is None else rec
    return hip.eval_stats(torch.from_numpy(z), torch.from_numpy(y), rec)


@pytest.mark.parametrize("B,K", O.SHAPES)
def test_record_matches_the_definitions(B, K):
    z, y = O.planted(B, K)
    O.assert_record(_run(z, y).numpy(), O.record(z, y), "cpu (%d, %d)" % (B, K))


def test_planted_ties_decide_the_hits():
    """What the plants are there for: the oracle itself separates the tie cases (so an implementation that breaks ties the other
    way cannot pass the comparison above)."""
    z, y = O.planted(7, 400)
    for clip, hits in ((0, (0, 1, 1)), (1, (1, 1, 1)), (4, (0, 1, 1)), (5, (0, 0, 1)), (6, (0, 0, 1))):
        r = O.record(z[clip:clip + 1], y[clip:clip + 1])
        assert tuple(r[2:5]) == hits, (clip, r[:6])
    r = O.record(z[2:4], y[2:4])
    assert r[5] == 2 and r[0] == 0 and r[1] == 0 and not r[O.HEAD:].any()


def test_fewer_classes_than_k_every_valid_clip_hits():
    z, y = O.planted(1, 3)
    got = _run(z, y).numpy()
    assert got[0] == 1 and got[2] == 0 and got[3] == 1 and got[4] == 1          # all equal, label 1: rank 1
    rng = np.random.default_rng(5)
    z = rng.standard_normal((9, 4)).astype(np.float32)
    y = rng.integers(0, 4, size=9).astype(np.int64)
    got = _run(z, y).numpy()
    assert got[4] == 9
    O.assert_record(got, O.record(z, y), "K = 4")


def test_labels_out_of_range_are_counted_apart():
    z = np.zeros((3, 5), dtype=np.float32)
    got = _run(z, np.array([-1, 5, 7], dtype=np.int64)).numpy()
    want = np.zeros(18)
    want[5] = 3
    assert np.array_equal(got, want)


def test_two_calls_accumulate_into_one_record():
    za, ya = O.planted(4, 5)
    zb, yb = O.planted(64, 5, seed=1)
    rec = _run(za, ya)
    rec = _run(zb, yb, rec)
    O.assert_record(rec.numpy(), O.record(zb, yb, O.record(za, ya)), "two calls")
    from video_distillation_amd import hip
    before = rec.clone()
    hip.eval_stats(torch.zeros((0, 5)), torch.zeros((0,), dtype=torch.int64), rec)          # B == 0 touches nothing
    assert torch.equal(rec, before)


def test_without_ties_the_hits_are_epochs_expressions():
    """utils.epoch: top-1 = (argmax == label), top-k = label among the last k of argsort."""
    g = torch.Generator().manual_seed(3)
    for B, K in ((64, 50), (7, 400), (33, 7)):
        out = torch.randn(B, K, generator=g)
        assert all(len(set(row.tolist())) == K for row in out)
        lab = torch.randint(0, K, (B,), generator=g)
        from video_distillation_amd import hip
        rec = hip.eval_stats(out, lab, hip.eval_stats_record(K))
        order = torch.argsort(out, dim=-1)
        matched = out.argmax(dim=-1) == lab
        assert rec[0] == B and rec[2] == int(matched.sum())
        for slot, k in ((3, 3), (4, 5)):
            assert rec[slot] == int((order[:, -k:] == lab[:, None]).any(dim=1).sum())
        assert torch.equal(rec[8:8 + K], torch.bincount(lab[matched], minlength=K).double())
        assert torch.equal(rec[8 + K:], torch.bincount(lab, minlength=K).double())
        want = torch.nn.functional.cross_entropy(out.double(), lab, reduction="sum")
        assert abs(float(rec[1]) - float(want)) <= 1e-12 * float(want)


def test_wrapper_refuses_a_record_of_the_wrong_size():
    from video_distillation_amd import hip
    with pytest.raises(ValueError):
        hip.eval_stats(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(17, dtype=torch.float64))
    with pytest.raises(ValueError):
        hip.eval_stats(torch.zeros(2, 5), torch.zeros(2, dtype=torch.int64), torch.zeros(18, dtype=torch.float32))
