"""vdr_regress_stats (csrc/regress_stats.hip, include/vd_regress.h) against numpy fp64 on the tensor ``frepo.soft_labels`` gives:
every count exactly, the sum of squared errors within the bound its fixed order of additions allows; the record's semantics
(it accumulates, B == 0 touches nothing, a second run gives the same bits); and against ``frepo.epoch('test')`` on the same logits.

The bound.  The kernel rounds every difference and every square on its own in fp64, as numpy does, so the TERMS are numpy's bit
for bit and only the additions differ from ``math.fsum``.  The order is fixed (the source's header comment): a lane adds its
``ceil(K / 64)`` terms, the 64 lanes of a clip meet in a 6-step butterfly, lane 0 adds the ``ceil(B / 16)`` clips of its wave, one
thread adds the 16 waves and then adds the batch to the record: no term passes through more than

    a = ceil(K / 64) + 6 + ceil(B / 16) + 16 + 1

additions, each with a relative error of at most 2^-53 on a partial sum of non-negative terms that never exceeds the total.  So
|rec[1] - fsum| <= a * 2^-53 * sum|terms| to first order; the three additions onto an exact 0.0 that ``a`` counts (a lane's, a
wave's and the batch's first) are exact and cover the oracle's own rounding (math.fsum: half a unit in the last place) and the
second-order remainder, which is smaller than a^2 * 2^-106 * sum."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 3), (17, 50), (16, 64), (33, 65), (256, 400)]
U = 2.0 ** -53


def chain(B, K):
    return -(-K // 64) + 6 + -(-B // 16) + 16 + 1


def batch(B, K, seed):
    """Logits with exact ties at lower and higher indices than the label (where K allows), one label at -1 and one at K (where B
    allows), otherwise labels over the whole range."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, K, generator=g)
    y = torch.randint(0, K, (B,), generator=g)
    if B >= 4 and K >= 3:
        y[0], y[1] = 1, 1
        z[0, 0] = z[0, 1]                      # an equal logit at a lower index: counts as above
        z[1, 2] = z[1, 1]                      # an equal logit at a higher index: does not
        z[2, :] = 0.25                         # every logit equal: the rank is the label itself
        y[3] = K - 1
        z[3, :] = -1.0
    if B >= 8:
        y[5], y[6] = -1, K
    return z, y


def oracle(z, y, K):
    """The record of one batch in numpy fp64 on frepo.soft_labels -> (rec with slot 1 by math.fsum, sum|terms|)."""
    from video_distillation_amd import frepo
    z64, yn = z.numpy().astype(np.float64), y.numpy()
    z32 = z.numpy()
    rec = np.zeros(8 + 2 * K)
    terms = []
    for b in range(z.shape[0]):
        lab = int(yn[b])
        if lab < 0 or lab >= K:
            rec[5] += 1
            continue
        soft = frepo.soft_labels(torch.tensor([lab]), K)[0].numpy()
        assert soft.dtype == np.float32
        d = z64[b] - soft.astype(np.float64)
        terms += (d * d).tolist()
        zy = z32[b, lab]
        above = int(np.sum(z32[b] > zy)) + int(np.sum(z32[b, :lab] == zy))
        rec[0] += 1
        rec[2] += above < 1
        rec[3] += above < 3
        rec[4] += above < 5
        rec[8 + lab] += above < 1
        rec[8 + K + lab] += 1
    rec[1] = math.fsum(terms)
    return rec, math.fsum(abs(t) for t in terms)


def check(got, want, bound, what):
    got = got.cpu().numpy()
    counts = [s for s in range(got.size) if s != 1]
    assert np.array_equal(got[counts], want[counts]), what
    err = abs(float(got[1]) - float(want[1]))
    print("%s: slot 1 error %.3e, bound %.3e (%.4f of it)" % (what, err, bound, err / bound if bound else 0.0))
    assert err <= bound, what


@pytest.mark.parametrize("B,K", SHAPES)
def test_the_record_against_numpy_fp64(B, K):
    from video_distillation_amd import hip
    z, y = batch(B, K, 100 + B + K)
    want, mag = oracle(z, y, K)
    rec = hip.eval_stats_record(K, "cuda")
    hip.regress_stats(z.cuda(), y.cuda(), rec)
    check(rec, want, chain(B, K) * U * mag, "B %d K %d" % (B, K))
    assert float(rec[6]) == 0.0 and float(rec[7]) == 0.0
    if B >= 8:
        assert float(rec[5]) == 2.0 and float(rec[0]) == B - 2
        assert float(rec[8 + K:].sum()) == B - 2
    # a second launch into a fresh record gives the same bits; a second launch into the same record accumulates
    again = hip.eval_stats_record(K, "cuda")
    hip.regress_stats(z.cuda(), y.cuda(), again)
    assert torch.equal(again.view(torch.int64), rec.view(torch.int64))
    z2, y2 = batch(B, K, 7)
    want2, mag2 = oracle(z2, y2, K)
    hip.regress_stats(z2.cuda(), y2.cuda(), rec)
    total = want + want2
    total[1] = math.fsum([want[1], want2[1]])
    # (the first batch's terms pass through one more addition, the second launch's onto the record; the oracle's two fsums and
    #  their sum are each rounded once more: two further units on the total)
    check(rec, total, (chain(B, K) + 1 + 2) * U * (mag + mag2), "B %d K %d, two launches" % (B, K))
    before = rec.clone()
    hip.regress_stats(z.cuda()[:0], y.cuda()[:0], rec)          # B == 0 leaves the record untouched
    assert torch.equal(rec.view(torch.int64), before.view(torch.int64))


def test_the_ties_follow_the_rank_rule():
    from video_distillation_amd import hip
    K = 6
    z = torch.tensor([[1.0, 1.0, 0.0, 0.0, 0.0, 0.0],          # label 1, an equal logit below it: rank 1
                      [0.0, 1.0, 1.0, 0.0, 0.0, 0.0],          # label 1, an equal logit above it: rank 0
                      [2.0, 2.0, 2.0, 2.0, 2.0, 2.0],          # label 4, all equal: rank 4 (top-5, not top-3)
                      [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]])         # label 5: rank 5
    y = torch.tensor([1, 1, 4, 5])
    rec = hip.regress_stats(z.cuda(), y.cuda(), hip.eval_stats_record(K, "cuda")).cpu()
    assert rec[:6].tolist()[0] == 4.0 and rec[2:6].tolist() == [1.0, 2.0, 3.0, 0.0]
    assert rec[8:8 + K].tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0] and rec[8 + K:].tolist() == [0.0, 2.0, 0.0, 0.0, 1.0, 1.0]


def test_a_nan_logit_ends_the_launch_with_counts_by_the_rule_and_a_nan_sum():
    from video_distillation_amd import hip
    B, K = 17, 50
    z, y = batch(B, K, 3)
    z[4, 7] = float("nan")                     # not the label's logit: every comparison with it is false
    y[4] = 9
    z[9, int(y[9])] = float("nan")             # the label's own logit: nothing compares above it, rank 0
    want, _ = oracle(z, y, K)
    rec = hip.regress_stats(z.cuda(), y.cuda(), hip.eval_stats_record(K, "cuda"))
    torch.cuda.synchronize()
    got = rec.cpu().numpy()
    assert math.isnan(got[1]) and math.isnan(want[1])
    counts = [s for s in range(got.size) if s != 1]
    assert np.array_equal(got[counts], want[counts]) and got[8 + int(y[9])] >= 1


def test_against_frepo_epoch_on_the_same_logits():
    """``epoch('test')`` with a network that returns the rows of a fixed logit table: the accuracy equals exactly, the loss to the
    rel 1e-5 tests/test_gpu_frepo_driver.py grants the fp32 sums of ``nn.MSELoss``."""
    import types
    from video_distillation_amd import frepo, hip
    K, N = 50, 37
    g = torch.Generator().manual_seed(9)
    table = torch.randn(N, K, generator=g).cuda()
    labels = torch.randint(0, K, (N,), generator=g)
    labels[:5] = table[:5].argmax(1).cpu()          # some hits for certain

    class Lookup(torch.nn.Module):
        def forward(self, x):
            return table.index_select(0, x.reshape(-1).long())
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(torch.arange(N, dtype=torch.float32), labels), batch_size=16)
    args = types.SimpleNamespace(device="cuda")
    net = Lookup()
    loss, acc = frepo.epoch('test', loader, net, None, torch.nn.MSELoss().cuda(), args, K)
    rec = hip.eval_stats_record(K, "cuda")
    with torch.no_grad():
        for x, lab in loader:
            hip.regress_stats(net(x.cuda()), lab.cuda(), rec)
    rec = rec.cpu()
    assert float(rec[0]) == N and float(rec[2]) / float(rec[0]) == acc and acc >= 5 / N
    assert float(rec[1]) / (K * float(rec[0])) == pytest.approx(loss, rel=1e-5)


def test_the_wrapper_checks_its_arguments_on_the_host():
    from video_distillation_amd import hip
    z, y = torch.zeros(2, 3).cuda(), torch.zeros(2, dtype=torch.int64).cuda()
    with pytest.raises(ValueError):
        hip.regress_stats(z, y, torch.zeros(8 + 5, dtype=torch.float64).cuda())          # a record of another K
    with pytest.raises(ValueError):
        hip.regress_stats(z, y[:1], hip.eval_stats_record(3, "cuda"))
    with pytest.raises(ValueError):
        hip.regress_stats(z, y.cpu(), hip.eval_stats_record(3, "cuda"))
    with pytest.raises(ValueError):
        hip.regress_stats(z, y.float(), hip.eval_stats_record(3, "cuda"))
