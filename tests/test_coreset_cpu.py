"""Coreset selection, CPU tier: the fp64 oracle against the reference's picks (fixture g18), the new C entry points' argument
checks, the Python API's argument errors and the driver's flags."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import coreset_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_coreset.npz"))


def _cases(z, gi):
    k = "g%d_" % gi
    for key in z.files:
        if key.startswith(k) and "_ipc" in key and "error" not in key:
            method, ipc = key[len(k):].rsplit("_ipc", 1)
            yield method, int(ipc), z[key]


@pytest.mark.parametrize("gi", [0, 1])
def test_fp64_restatement_reproduces_the_reference_picks(g18, gi):
    counts = g18["g%d_counts" % gi]
    seen = set()
    for method, ipc, picks in _cases(g18, gi):
        assert picks.shape == (len(counts), ipc)
        for c in range(len(counts)):
            G = g18["g%d_gram_%d" % (gi, c)]
            assert G.shape == (counts[c], counts[c])
            np.testing.assert_allclose(G, G.T, rtol=0, atol=1e-12 * np.abs(G).max())
            mode = "reference" if method == "k-center" else "greedy"
            want, _, _ = O.select(G, ipc, method, kcenter=mode)
            assert list(picks[c]) == want, (method, ipc, c)
            if method == "k-center" and ipc == 1:          # the greedy algorithm's first pick is the reference's
                assert O.kcenter_greedy(G, 1)[0] == want
        seen.add((method, ipc))
    assert {("herding", 1), ("herding", 3), ("k-center", 1), ("k-center", 2)} <= seen
    assert ("herding", int(min(counts))) in seen
    assert "must match the size of tensor" in str(g18["g%d_kcenter_ipc3_error" % gi])


@pytest.mark.parametrize("gi", [0, 1])
def test_fixture_weights_are_the_pinned_initialisation(g18, gi):
    from oracle import ref_cpu as R
    params = R.init_params(int(g18["g%d_wseed" % gi]), num_classes=len(g18["g%d_counts" % gi]))
    chk = np.array([float(p.double().sum()) for p in params])
    np.testing.assert_allclose(chk, g18["g%d_param_checksum" % gi], rtol=1e-12, atol=1e-9)


def test_greedy_kcenter_is_farthest_point():
    rng = np.random.default_rng(3)
    f = rng.standard_normal((40, 17))
    G = O.centred_gram(f)
    picks, _, _ = O.kcenter_greedy(G, 10)
    m = f.mean(0)
    assert picks[0] == int(np.argmin(((f - m) ** 2).sum(1)))
    for t in range(1, 10):
        d = np.min(((f[:, None, :] - f[None, picks[:t], :]) ** 2).sum(-1), axis=1)
        d[picks[:t]] = -np.inf
        assert picks[t] == int(np.argmax(d))
    # herding on the Gram equals herding on the features (distill_coreset.py's criterion)
    hp, _, _ = O.herding(G, 10)
    sel, left = [], list(range(40))
    for i in range(10):
        det = m * (i + 1) - (f[sel].sum(0) if sel else 0)
        j = int(np.argmin(np.linalg.norm(det - f[left], axis=1)))
        sel.append(left.pop(j))
    assert hp == sel


def _lib():
    from video_distillation_amd import hip
    hip.build()
    return hip.bind(hip.LIB_PATH)


def test_coreset_entry_points_check_arguments_before_any_device_call():
    L = _lib()
    assert L.vd_coreset_workspace_bytes(3, 10) == 3 * 10 * 10 * 8
    assert L.vd_coreset_workspace_bytes(0, 10) == -2 and L.vd_coreset_workspace_bytes(3, 0) == -2
    assert L.vd_coreset_workspace_bytes(1, 5000) == -2
    p = ctypes.c_void_p(16)           # never dereferenced: every call below is refused before the device is touched
    N = None
    args = lambda **kw: [kw.get(k, d) for k, d in (("feats", p), ("dim", 256), ("offsets", p), ("counts", p), ("nclass", 3),
                                                   ("max_count", 10), ("ipc", 2), ("method", 0), ("out", p), ("ws", p),
                                                   ("wsb", ctypes.c_int64(2400)), ("stream", N))]
    for k in ("feats", "offsets", "counts", "out", "ws"):
        assert L.vd_coreset_select(*args(**{k: N})) == -1, k
    for kw in ({"dim": 0}, {"dim": 8193}, {"nclass": 0}, {"max_count": 0}, {"max_count": 4097}, {"ipc": 0}, {"method": 2},
               {"method": -1}, {"wsb": ctypes.c_int64(2399)}):
        assert L.vd_coreset_select(*args(**kw)) == -2, kw


def test_select_argument_errors_need_no_gpu():
    from video_distillation_amd import coreset
    f = torch.zeros(12, 8)
    with pytest.raises(ValueError, match="fewer than ipc"):
        coreset.select(f, [5, 7], [0, 5], 6, "herding")
    with pytest.raises(NotImplementedError):
        coreset.select(f, [5, 7], [0, 5], 1, "random")
    with pytest.raises(ValueError, match="distill_coreset.py"):
        coreset.select(f, [5, 7], [0, 5], 3, "k-center", kcenter="reference")
    with pytest.raises(ValueError):
        coreset.select(f, [5, 7], [0, 5], 1, "k-center", kcenter="nearest")
    with pytest.raises(RuntimeError, match="HIP device"):      # valid arguments on a CPU tensor: no CPU path
        coreset.select(f, [5, 7], [0, 5], 2, "herding")


def test_run_coreset_parser_defaults_are_the_reference_script_defaults():
    from video_distillation_amd import run_coreset
    a = run_coreset.build_parser().parse_args([])
    # distill_coreset.py's argparse block
    ref = {"dataset": "miniUCF101", "method": "k-center", "model": "ConvNet3D", "ipc": 1, "eval_mode": "S", "num_eval": 5,
           "epoch_eval_train": 1000, "lr_net": 0.001, "batch_train": 256, "data_path": "distill_utils/data",
           "pretrained_path": None, "num_workers": 8, "save_path": ".", "frames": 16, "preload": False}
    assert {k: getattr(a, k) for k in ref} == ref
    assert a.kcenter == "greedy" and a.log_file is None and a.data_file is None and a.im_size == 112


def test_run_coreset_refuses_several_ranks(monkeypatch):
    from video_distillation_amd import run_coreset
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one rank"):
        run_coreset.main(["--dataset", "synthetic"])
