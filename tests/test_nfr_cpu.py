"""include/vd_nfr.h without a GPU (its binding and hashes: tests/test_cabi.py): argument errors come back before any device call,
the workspace is large enough for what it carries, and the two forms of the fp64 oracle (tests/nfr_oracle.py) agree within the
bar and meet the fixture the reference's own ``PoolElement.nfr`` wrote (tools/gen_golden.py g18)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import nfr_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


BAD_DIMS = [(0, 1, 1, 1), (1025, 1, 1, 1), (-1, 1, 1, 1), (4, 0, 4, 4), (4, -3, 4, 4), (4, 4, 0, 4), (4, 4, -1, 4), (4, 4, 4, 0), (4, 4, 4, -2)]


def test_argument_errors_come_back_before_any_device_call():
    """No device is present here: a call that reached HIP would not return -1."""
    from video_distillation_amd import hip
    lib = hip.lib()
    buf = (ctypes.c_double * 64)()
    a = ctypes.addressof(buf)
    for k in range(5):          # each pointer of forward in turn
        args = [a, a, a, a, a]
        args[k] = None
        assert lib.vdn_nfr_forward(args[0], args[1], args[2], 2, 2, 2, 2, 1e-6, args[3], args[4], None) == -1, k
    for k in range(6):          # and of backward
        args = [a, a, a, a, a, a]
        args[k] = None
        assert lib.vdn_nfr_backward(args[0], args[1], args[2], 2, 2, 2, 2, 1e-6, args[3], args[4], args[5], None) == -1, k
    for n, m, d, c in BAD_DIMS:
        assert lib.vdn_nfr_forward(a, a, a, n, m, d, c, 1e-6, a, a, None) == -1, (n, m, d, c)
        assert lib.vdn_nfr_backward(a, a, a, n, m, d, c, 1e-6, a, a, a, None) == -1, (n, m, d, c)
        assert lib.vdn_nfr_workspace_bytes(n, m, d, c) == -1, (n, m, d, c)


@pytest.mark.parametrize("n,m,d,c", [(1, 1, 1, 1), (50, 512, 2048, 50), (400, 512, 256, 400), (1024, 7, 3, 5), (3, 2 ** 20, 9, 2)])
def test_the_workspace_holds_the_factor_the_solution_the_cross_kernel_and_the_status(n, m, d, c):
    from video_distillation_amd import hip
    got = hip.lib().vdn_nfr_workspace_bytes(n, m, d, c)
    assert got >= 8 * (n * n + n * c + m * n) + 8 and got % 8 == 0


def test_the_python_wrappers_refuse_on_the_host():
    from video_distillation_amd import hip, nfr
    fs, ys, ft = torch.zeros(3, 4), torch.zeros(3, 2), torch.zeros(5, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        hip.nfr_forward(fs, ys, ft)
    with pytest.raises(RuntimeError, match="no CPU path"):
        nfr.nfr_pred(fs, ys, ft)
    with pytest.raises(ValueError):
        hip.nfr_forward(fs, ys, torch.zeros(5, 3))
    with pytest.raises(ValueError):
        hip.nfr_forward(fs, torch.zeros(4, 2), ft)
    with pytest.raises(ValueError):
        nfr.nfr_pred(fs, ys, ft.requires_grad_(True))
    with pytest.raises(ValueError):
        nfr.nfr_pred(fs.double(), ys, torch.zeros(5, 4))


@pytest.mark.parametrize("case", O.CASES, ids=O.case_id)
def test_the_two_forms_of_the_oracle_agree_within_the_bar(case):
    fs, ys, ft, R = O.inputs(case)
    assert float(fs.abs().max()) > 0
    a, b = O.by_autograd(fs, ys, ft, R, case[4]), O.by_formulas(fs, ys, ft, R, case[4])
    c = O.cond(fs, case[4])
    errs = [O.rel_l2(y, x) for x, y in zip(a, b)]
    print("%s: cond %.3e, bar %.3e, rel-L2 of (b) to (a): %s" % (O.case_id(case), c, O.bar(c), ["%.2e" % e for e in errs]))
    assert max(errs) <= O.bar(c)


def test_the_measured_condition_numbers_are_those_the_cases_were_chosen_for():
    conds = {O.case_id(case): O.cond(O.inputs(case)[0], case[4]) for case in O.CASES}
    assert 1e6 < conds[O.case_id(O.CASES[6])] < 1.3e7 and 1e6 < conds[O.case_id(O.CASES[7])] < 4.1e7          # n > d: bounded by 1 + n / reg
    assert conds[O.case_id(O.CASES[8])] > 1e6 > conds[O.case_id(O.CASES[9])]          # duplicated rows: reg 1e-6 / 1e-3
    assert max(O.bar(c) for c in conds.values()) < 2.0 ** -24          # every bar is below one fp32 rounding


def test_form_a_meets_the_fixture_of_the_reference():
    """tests/golden/nfr/values.npz: ``PoolElement.nfr`` of the reference on double inputs (stand-in model: embed = identity).
    Its lambda passes through a float32 ``torch.eye``; the oracle's is fp64.  A relative 2^-24 = 6e-8 in lambda moves Z by at
    most lambda |A^-1| 2^-24 <= 6e-8 relative, and the products around Z may lose an order of magnitude to cancellation: the bar
    is 1e-6 rel-L2, not the fp64 bar."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "nfr", "values.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "nfr", "values.npz")) < 100 * 1024
    for tag, index in zip("abcd", z["cases"]):
        case = O.CASES[int(index)]
        fs, ys, ft, R = O.inputs(case)
        for name, t in (("feat_syn", fs), ("y_syn", ys), ("feat_tar", ft), ("g_pred", R)):
            assert np.array_equal(z["%s_%s" % (tag, name)], t.double().numpy()), (tag, name)
        assert float(z[tag + "_reg"]) == case[4]
        got = O.by_autograd(fs, ys, ft, R, case[4])
        errs = [O.rel_l2(g, z["%s_%s" % (tag, name)]) for g, name in zip(got, ("pred", "g_feat_syn", "g_y_syn"))]
        print("%s against the reference: rel-L2 %s" % (O.case_id(case), ["%.2e" % e for e in errs]))
        assert max(errs) <= 1e-6, (O.case_id(case), errs)


def test_closed_form_at_one_synthetic_clip():
    """n = 1: A = (1 + |reg|) f.f, so pred[r] = (f_t[r].f) / ((1 + |reg|) f.f) y."""
    g = torch.Generator().manual_seed(3)
    f, y, ft, R = torch.rand(1, 6, generator=g) + 0.5, torch.randn(1, 4, generator=g), torch.randn(5, 6, generator=g), torch.randn(5, 4, generator=g)
    reg = 1e-3
    want = (ft.double() @ f.double().t()) / ((1.0 + reg) * float((f.double() ** 2).sum())) * y.double()
    for form in (O.by_autograd, O.by_formulas):
        assert O.rel_l2(form(f, y, ft, R, reg)[0], want) < 1e-14


def test_no_file_of_the_package_imports_the_oracle():
    src = open(os.path.join(ROOT, "video_distillation_amd", "nfr.py")).read()
    assert "import oracle" not in src and "from oracle" not in src and "linalg.solve" not in src
