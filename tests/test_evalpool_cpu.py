"""evalpool.evaluate_pool on the CPU: the unit-to-rank rule, and gloo worlds of 2 and 3 ranks against one rank -- the same call
gives the same dict on every rank, bit-equal to the one-rank run's in every record slot and derived number (oracle networks
from tests/cpu_backend.py; hip.eval_stats takes its torch fp64 branch on CPU tensors)."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

C, T, S = 3, 8, 64          # (the smallest clip ConvNet3D takes: three stride-2 convolutions and three poolings)
SEED = 20240611


# ------------------------------------------------------------------------------------------------ the assignment rule
def test_every_unit_is_assigned_once_and_loads_are_even():
    from video_distillation_amd import evalpool
    for world in range(1, 17):
        for num_eval in range(1, 7):
            plan = evalpool.assignment(num_eval, world)
            assert len(plan["train"]) == num_eval and all(len(row) == 3 for row in plan["test"]) and len(plan["test"]) == num_eval
            units = [(i, p, plan["test"][i][p]) for i in range(num_eval) for p in range(3)]
            assert len(units) == 3 * num_eval and all(0 <= r < world for _, _, r in units)
            assert all(evalpool.unit_rank(i, p, num_eval, world) == r for i, p, r in units)          # one rank per unit
            assert all(0 <= plan["train"][i] < world and plan["train"][i] == i % world for i in range(num_eval))
            load = np.bincount([r for _, _, r in units], minlength=world)
            assert load.sum() == 3 * num_eval
            if world <= 3 * num_eval:
                assert load.max() - load.min() <= 1, (world, num_eval, load)
            # "no unit leaves its owner when world divides num_eval" is num_eval % world == 0 (world 1 included).  The issue's
            # check list wrote the condition the other way round (world % num_eval == 0), which the rule it fixes,
            # (i + p * num_eval) % world, cannot meet: world 2, num_eval 1 sends pass 1 to rank 1.  What does hold in that
            # case is asserted as well: every pass stays on a rank congruent to the owner modulo num_eval.
            if num_eval % world == 0:
                assert all(r == plan["train"][i] for i, _, r in units), (world, num_eval)
            if world % num_eval == 0:
                assert all(r % num_eval == plan["train"][i] % num_eval for i, _, r in units), (world, num_eval)


def test_unit_seeds_are_distinct():
    from video_distillation_amd import evalpool
    seeds = {evalpool.unit_seed(s, i, k) for s in (0, 1, SEED) for i in range(6) for k in range(4)}
    assert len(seeds) == 3 * 6 * 4 and all(0 <= s < 2 ** 63 for s in seeds)


# ------------------------------------------------------------------------------------------------ the run
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _problem():
    g = torch.Generator().manual_seed(99)
    images = torch.randn(2 * C, T, 3, S, S, generator=g)
    labels = torch.arange(C).repeat_interleave(2)
    test_x = torch.randn(7, T, 3, S, S, generator=g)
    test_y = torch.randint(0, C, (7,), generator=g)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test_x, test_y), batch_size=4, shuffle=False)
    args = types.SimpleNamespace(device="cpu", lr_net=0.01, epoch_eval_train=2, batch_train=4, model="ConvNet3D", eval_mode="SS")
    return images, labels, loader, args


def _make_net(i):
    from oracle import ref_cpu as R
    from tests.cpu_backend import _OracleNet
    return _OracleNet(R.init_params(100 + i, 3, C))


def _failing_make_net(i):
    if dist.get_rank() == 1:
        raise ValueError("planted failure on rank 1")
    return _make_net(i)


def _plain(result):
    """The dict without its wall times, tensors as nested lists of exact float reprs."""
    out = {k: v for k, v in result.items() if k != "times"}
    out["records"] = [float(v).hex() for v in result["records"].reshape(-1).tolist()]
    for k in ("acc_test", "loss_test", "top1", "top3", "top5", "acc_train", "loss_train"):
        out[k] = [float(v).hex() for v in result[k]]
    out["mean"], out["std"] = float(result["mean"]).hex(), float(result["std"]).hex()
    out["acc_per_class"] = [[None if v is None else float(v).hex() for v in row] for row in result["acc_per_class"]]
    return out


def _worker(rank, world, port, q, num_eval, fail):
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    from video_distillation_amd import evalpool
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        images, labels, loader, args = _problem()
        weights = {}
        try:
            got = evalpool.evaluate_pool(_failing_make_net if fail else _make_net, images, labels, loader, args, num_eval=num_eval,
                                         seed=SEED, mode='none', rank=rank, world=world, num_classes=C,
                                         on_trained=lambda i, net: weights.__setitem__(i, evalpool.flat_weights(net).numpy().tobytes()))
            q.put((rank, "ok", _plain(got), got["times"], weights))
        except Exception as e:      # noqa: BLE001 -- the failure test reports what every rank raised
            q.put((rank, "raised", "%s: %s" % (type(e).__name__, e), None, None))
    finally:
        if world > 1:
            dist.destroy_process_group()


def _spawn(world, num_eval, fail=False, timeout=120):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, num_eval, fail)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        got = sorted((q.get(timeout=timeout) for _ in range(world)), key=lambda t: t[0])
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    return got


_ONE = {}


def _one_rank(num_eval):
    """The one-rank run of a ``num_eval``: computed once, shared by the tests below."""
    if num_eval not in _ONE:
        (_, status, plain, times, weights), = _spawn(1, num_eval)
        assert status == "ok", plain
        _ONE[num_eval] = (plain, times, weights)
    return _ONE[num_eval]


def test_one_rank_result_is_what_the_records_say():
    plain, times, weights = _one_rank(2)
    assert plain["num_eval"] == 2 and plain["world"] == 1 and plain["num_classes"] == C
    assert plain["assignment"] == {"train": [0, 0], "test": [[0, 0, 0], [0, 0, 0]]}
    rec = np.array([float.fromhex(v) for v in plain["records"]]).reshape(2, 4, 8 + 2 * C)
    assert np.array_equal(rec[:, :3, 0], np.full((2, 3), 7.0)) and plain["test_clips"] == [21, 21]
    assert not rec[:, :3, 5:8].any()
    for i in range(2):
        assert float.fromhex(plain["acc_test"][i]) == rec[i, :3, 2].sum() / 21
        assert float.fromhex(plain["loss_test"][i]) == rec[i, :3, 1].sum() / 21
        assert float.fromhex(plain["loss_train"][i]) == rec[i, 3, 0] and float.fromhex(plain["acc_train"][i]) == rec[i, 3, 1]
        assert np.array_equal(rec[i, :3, 8 + C:].sum(0), 3 * np.bincount(_problem()[2].dataset.tensors[1].numpy(), minlength=C))
    accs = [float.fromhex(v) for v in plain["acc_test"]]
    assert float.fromhex(plain["mean"]) == float(np.mean(accs)) and float.fromhex(plain["std"]) == float(np.std(accs))
    assert len(times["train_s"]) == 2 and all(t > 0 for t in times["train_s"]) and all(t > 0 for row in times["test_pass_s"] for t in row)
    assert sorted(weights) == [0, 1] and weights[0] != weights[1]          # two different networks were trained
    # the same passes give the same record: the test set is fixed and evaluation draws nothing
    assert np.array_equal(rec[:, 0], rec[:, 1]) and np.array_equal(rec[:, 0], rec[:, 2])


@pytest.mark.parametrize("world,num_eval", [(2, 3), (3, 2)])
def test_gloo_worlds_are_bit_equal_to_one_rank(world, num_eval):
    """world 2 / num_eval 3: networks 0 and 2 on rank 0, 1 on rank 1, units spread 5 + 4.  world 3 / num_eval 2: rank 2 owns no
    network and tests pass 1 of network 0 and pass 2 of network 1 -- the weights must travel."""
    from video_distillation_amd import evalpool
    plan = evalpool.assignment(num_eval, world)
    moved = [(i, p) for i in range(num_eval) for p in range(3) if plan["test"][i][p] != plan["train"][i]]
    assert moved
    if world == 3:
        assert 2 not in plan["train"] and 2 in [r for row in plan["test"] for r in row]
    one, _, one_weights = _one_rank(num_eval)
    got = _spawn(world, num_eval)
    owned = {}
    for rank, status, plain, times, weights in got:
        assert status == "ok", plain
        assert plain == dict(one, world=world, assignment=plan), "rank %d of %d differs from the one-rank run" % (rank, world)
        assert sorted(weights) == [i for i in range(num_eval) if plan["train"][i] == rank]
        owned.update(weights)
        assert times == got[0][3]                  # the times are all-reduced too: one dict everywhere
    assert owned == one_weights                    # the trained weights do not depend on the rank that trained them


def test_a_rank_that_raises_makes_every_rank_raise():
    got = _spawn(3, 2, fail=True, timeout=60)
    assert [status for _, status, _, _, _ in got] == ["raised"] * 3, got
    assert "planted failure on rank 1" in got[1][2]
    assert all("another rank failed in the train phase" in got[r][2] for r in (0, 2)), got


def test_run_dm_keeps_rank0_evaluation_by_default():
    from video_distillation_amd import run_dm
    args = run_dm.build_parser().parse_args([])
    assert args.eval_ranks == "rank0" and args.eval_seed is None
    args = run_dm.build_parser().parse_args(["--eval_ranks", "all", "--eval_seed", "7"])
    assert args.eval_ranks == "all" and args.eval_seed == 7
    with pytest.raises(SystemExit):
        run_dm.build_parser().parse_args(["--eval_ranks", "some"])
