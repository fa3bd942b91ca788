"""evalpool.evaluate_pool with the HIP kernels underneath, on a one-GPU box: three ranks on device 0 over gloo (spawned by
torch.distributed.run like the one-device tests of tests/test_gpu_collectives.py) against one rank, in the ordered mode
(VD_DETERMINISTIC=1: the training step's sums have a fixed order, so records and trained weights are compared bit for bit;
with the switch off the fp32 atomics' order may move a count, and nothing is asserted there).  And ``run_dm --eval_ranks all``
at two ranks: its logged accuracy is evaluate_pool's one-rank result under the same seed."""
import json
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "evalpool_gpu_tool.py")


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def _env():
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VD_DETERMINISTIC="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        e.pop(k, None)
    return e


def _ranks(world, args, timeout=300):
    cmd = [sys.executable, TOOL] if world == 1 else [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
                                                     str(world), "--master-addr", "127.0.0.1", "--master-port", _free_port(), TOOL]
    out = subprocess.run(cmd + args, cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return out


def test_three_ranks_on_one_device_are_bit_equal_to_one_rank(tmp_path):
    """num_eval 2 at world 3: rank 2 owns no network and runs pass 1 of network 0 and pass 2 of network 1, rank 0 also tests
    network 1 and rank 1 network 0 -- both networks' weights travel."""
    one, three = str(tmp_path / "one"), str(tmp_path / "three")
    with ThreadPoolExecutor(max_workers=2) as ex:          # five processes on the card with the launcher
        jobs = [ex.submit(_ranks, 1, ["pool", "--out", one]), ex.submit(_ranks, 3, ["pool", "--out", three])]
        for j in jobs:
            j.result()
    want = json.load(open(one + ".rank0.json"))
    assert want["assignment"] == {"train": [0, 0], "test": [[0, 0, 0], [0, 0, 0]]} and want["test_clips"] == [21, 21]
    assert sorted(want["weights_sha256"]) == ["0", "1"] and want["weights_sha256"]["0"] != want["weights_sha256"]["1"]
    got = [json.load(open("%s.rank%d.json" % (three, r))) for r in range(3)]
    assert got[0]["assignment"] == {"train": [0, 1], "test": [[0, 2, 1], [1, 0, 2]]}
    trained = {}
    for r, g in enumerate(got):
        trained.update(g["weights_sha256"])
        for k in want:
            if k not in ("world", "assignment", "weights_sha256"):
                assert g[k] == want[k], "rank %d: %s differs from the one-rank run" % (r, k)
    assert sorted(got[0]["weights_sha256"]) == ["0"] and sorted(got[1]["weights_sha256"]) == ["1"] and not got[2]["weights_sha256"]
    assert trained == want["weights_sha256"]           # final weights of both networks, bit for bit


def test_run_dm_eval_ranks_all_logs_the_pool_accuracy(tmp_path):
    from tests import evalpool_gpu_tool as tool
    data, log, syn, out = (str(tmp_path / n) for n in ("toy.pt", "log.jsonl", "syn.pt", "one"))
    tool.toy_data_file(data)
    _ranks(2, ["run_dm", "--data_file", data, "--log_file", log, "--save_syn", syn, "--eval_seed", "23"])
    lines = [json.loads(l) for l in open(log)]
    accs = [l for l in lines if "Accuracy/ConvNet3D" in l]
    assert len(accs) == 1 and accs[0]["step"] == 0
    assert {"eval_ranks": "all", "eval_seed": 23, "world": 2} in lines
    _ranks(1, ["pool_on", "--data_file", data, "--syn", syn, "--eval_seed", "23", "--out", out])
    want = json.load(open(out + ".rank0.json"))
    assert accs[0]["Accuracy/ConvNet3D"] == want["mean_float"] and accs[0]["Std/ConvNet3D"] == float.fromhex(want["std"])
    assert accs[0]["Max_Accuracy/ConvNet3D"] == (want["mean_float"] if want["mean_float"] > 0 else 0.0)
