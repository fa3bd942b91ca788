"""vd_eval_stats (csrc/eval_stats.hip) through the C ABI against the numpy restatement of the record's definitions
(tests/eval_stats_oracle.py), on the shapes and planted ties of the CPU test plus the largest evaluation batch (256 x 400):
counts exactly, the cross-entropy sum within 1e-12 relative, two runs bitwise equal, argument errors before any launch."""
import ctypes

import numpy as np
import pytest
import torch

from tests import eval_stats_oracle as O

pytestmark = pytest.mark.gpu

VP = ctypes.c_void_p


def _call(z, y, B, K, rec):
    from video_distillation_amd import hip
    rc = hip.lib().vd_eval_stats(VP(0 if z is None else z.data_ptr()), VP(0 if y is None else y.data_ptr()), B, K,
                                 VP(0 if rec is None else rec.data_ptr()), hip.stream_ptr())
    torch.cuda.synchronize()
    return rc


def _run(z, y, rec=None):
    zd, yd = torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda()
    rec = torch.zeros(O.HEAD + 2 * z.shape[1], dtype=torch.float64, device="cuda") if rec is None else rec
    assert _call(zd, yd, z.shape[0], z.shape[1], rec) == 0
    return rec


@pytest.mark.parametrize("B,K", O.SHAPES + ((256, 400),))
def test_record_matches_the_definitions_and_is_bitwise_reproducible(B, K):
    z, y = O.planted(B, K)
    got = _run(z, y)
    O.assert_record(got.cpu().numpy(), O.record(z, y), "gpu (%d, %d)" % (B, K))
    again = _run(z, y)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))


def test_two_calls_accumulate_into_one_record():
    za, ya = O.planted(4, 5)
    zb, yb = O.planted(64, 5, seed=1)
    rec = _run(zb, yb, _run(za, ya))
    O.assert_record(rec.cpu().numpy(), O.record(zb, yb, O.record(za, ya)), "gpu, two calls")


def test_wrapper_sends_device_tensors_to_the_kernel_and_agrees_with_its_cpu_branch():
    from video_distillation_amd import hip
    z, y = O.planted(64, 50)
    calls = []

    def spy(code, what):
        calls.append(what)
        return real(code, what)
    real, hip.check = hip.check, spy
    try:
        dev = hip.eval_stats(torch.from_numpy(z).cuda(), torch.from_numpy(y).cuda(), hip.eval_stats_record(50, "cuda"))
        torch.cuda.synchronize()
    finally:
        hip.check = real
    assert calls == ["vd_eval_stats"]
    cpu = hip.eval_stats(torch.from_numpy(z), torch.from_numpy(y), hip.eval_stats_record(50))
    O.assert_record(dev.cpu().numpy(), cpu.numpy(), "wrapper: device against cpu branch")


def test_argument_errors_and_the_empty_batch():
    z = torch.zeros(4, 5, device="cuda")
    y = torch.zeros(4, dtype=torch.int64, device="cuda")
    rec = torch.full((18,), 3.0, dtype=torch.float64, device="cuda")
    for args in ((z, y, -1, 5, rec), (z, y, 4, 0, rec), (z, y, 4, -2, rec), (None, y, 4, 5, rec), (z, None, 4, 5, rec),
                 (z, y, 4, 5, None)):
        assert _call(*args) == -1, args[2:4]
    assert _call(z, y, 0, 5, rec) == 0 and _call(None, None, 0, 5, None) == 0
    assert np.array_equal(rec.cpu().numpy(), np.full(18, 3.0))          # nothing was touched by any of the calls above
