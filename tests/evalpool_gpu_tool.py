"""Child processes of tests/test_gpu_evalpool.py (one per rank; all ranks on device 0, exchange over gloo -- RCCL refuses two
ranks on one device, as in tests/test_gpu_collectives.py).

    pool    --out PREFIX --num_eval N          evaluate_pool on the toy problem below; every rank writes PREFIX.rank<r>.json
    run_dm  --data_file F --log_file L --save_syn S --eval_seed E     run_dm --eval_ranks all on a toy data file; rank 0 saves
                                                                      the synthetic set it evaluated
    pool_on --data_file F --syn S --eval_seed E --out PREFIX          evaluate_pool, one rank, on that saved set
"""
import argparse
import hashlib
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch                    # noqa: E402
import torch.distributed as dist      # noqa: E402

C, T, S = 3, 8, 64
DM_ARGS = ["--ipc", "1", "--Iteration", "0", "--eval_it", "1", "--num_eval", "2", "--epoch_eval_train", "2", "--batch_real", "8",
           "--batch_train", "4", "--frames", str(T), "--im_size", str(S), "--eval_ranks", "all"]


def toy_problem():
    """C = 3 at 8 x 64 x 64: two training clips per class, 7 test clips in batches of 4 (a short last batch); epoch_eval_train 2
    puts the learning-rate switch (after epoch 2) inside the three epochs."""
    g = torch.Generator().manual_seed(99)
    images = torch.randn(2 * C, T, 3, S, S, generator=g).cuda()
    labels = torch.arange(C).repeat_interleave(2).cuda()
    test_x = torch.randn(7, T, 3, S, S, generator=g)
    test_y = torch.randint(0, C, (7,), generator=g)
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(test_x, test_y), batch_size=4, shuffle=False)
    args = types.SimpleNamespace(device="cuda:0", lr_net=0.01, epoch_eval_train=2, batch_train=4, model="ConvNet3D", eval_mode="SS")
    return images, labels, loader, args


def toy_data_file(path):
    g = torch.Generator().manual_seed(7)
    torch.save({"clips": torch.randn(8 * C, T, 3, S, S, generator=g), "labels": torch.arange(C).repeat_interleave(8),
                "test_clips": torch.randn(7, T, 3, S, S, generator=g), "test_labels": torch.randint(0, C, (7,), generator=g)}, path)


def exact(result, weights):
    """The result dict with every float as its exact hex string (the wall times left out)."""
    out = {k: v for k, v in result.items() if k not in ("times", "records")}
    out["records"] = [float(v).hex() for v in result["records"].reshape(-1).tolist()]
    for k in ("acc_test", "loss_test", "top1", "top3", "top5", "acc_train", "loss_train"):
        out[k] = [float(v).hex() for v in result[k]]
    out["mean"], out["std"] = float(result["mean"]).hex(), float(result["std"]).hex()
    out["acc_per_class"] = [[None if v is None else float(v).hex() for v in row] for row in result["acc_per_class"]]
    out["mean_float"] = result["mean"]
    out["weights_sha256"] = weights
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["pool", "run_dm", "pool_on"])
    ap.add_argument("--out"); ap.add_argument("--num_eval", type=int, default=2)
    ap.add_argument("--data_file"); ap.add_argument("--log_file"); ap.add_argument("--save_syn"); ap.add_argument("--syn")
    ap.add_argument("--eval_seed", type=int, default=11)
    a = ap.parse_args()
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    os.environ["LOCAL_RANK"] = "0"             # every rank on device 0
    torch.cuda.set_device(0)
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    from video_distillation_amd import evalpool, hip
    assert hip.deterministic(), "run with VD_DETERMINISTIC=1: the comparison is bit for bit"
    weights = {}

    def keep(i, net):
        weights[str(i)] = hashlib.sha256(evalpool.flat_weights(net).cpu().numpy().tobytes()).hexdigest()
    try:
        if a.what == "pool":
            images, labels, loader, eargs = toy_problem()
            got = evalpool.evaluate_pool(None, images, labels, loader, eargs, num_eval=a.num_eval, seed=a.eval_seed, mode='none',
                                         rank=rank, world=world, num_classes=C, on_trained=keep)
            with open("%s.rank%d.json" % (a.out, rank), "w") as f:
                json.dump(exact(got, weights), f)
        elif a.what == "run_dm":
            from video_distillation_amd import run_dm
            real = evalpool.evaluate_pool

            def spy(make_net, images_train, *rest, **kw):
                if rank == 0:
                    torch.save(images_train.detach().cpu(), a.save_syn)
                return real(make_net, images_train, *rest, **kw)
            evalpool.evaluate_pool = spy
            args = run_dm.build_parser().parse_args(DM_ARGS + ["--data_file", a.data_file, "--eval_seed", str(a.eval_seed), "--save_path",
                                                               os.path.dirname(a.log_file)] + (["--log_file", a.log_file]))
            run_dm.run(args)
        else:
            blob = torch.load(a.data_file, map_location="cpu")
            loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(blob["test_clips"].float(), blob["test_labels"].long()),
                                                 batch_size=64, shuffle=False)                    # as run_dm.load_data builds it
            eargs = types.SimpleNamespace(device="cuda:0", lr_net=0.01, epoch_eval_train=2, batch_train=4, model="ConvNet3D", eval_mode="SS")
            syn = torch.load(a.syn, map_location="cpu").cuda()
            got = evalpool.evaluate_pool(None, syn, torch.arange(C), loader, eargs, num_eval=2, seed=a.eval_seed, mode='none',
                                         num_classes=C, on_trained=keep)
            with open("%s.rank0.json" % a.out, "w") as f:
                json.dump(exact(got, weights), f)
        torch.cuda.synchronize()
    finally:
        if world > 1:
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
