"""On-disk artefacts of the reference's DM drivers (SURVEY 5 "Checkpoint / resume", 8(f)-4).

The reference is save-only; file names and tensor layouts are the contract:
  * ``images_{it}.pt`` / ``images_best.pt``  -- ``torch.save(image_syn.cpu())``, (C*ipc,T,3,H,W)
    (distill_baseline.py:324-332);
  * ``dynamic_{it}.pt`` / ``dynamic_best.pt`` -- dynamic memory flattened to (C*dpc,T,1,H,W),
    ``hal_{it}.pt`` / ``weights_best.pt`` -- ``ModuleList[Conv3DNet].state_dict()`` i.e. keys
    ``{i}.encoder.weight`` / ``{i}.encoder.bias`` (distill_s2d_ms.py:362-392);
  * static memory is LOADED from ``torch.load(path)["image"]`` (distill_s2d_ms.py:96-99).
"""
from __future__ import annotations

import os
from typing import Dict, Sequence

import torch


def save_images(save_dir: str, it: int, image_syn: torch.Tensor, best: bool = False) -> str:
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, "images_%d.pt" % it)
    torch.save(image_syn.detach().cpu(), path)
    if best:
        torch.save(image_syn.detach().cpu(), os.path.join(save_dir, "images_best.pt"))
    return path


def save_s2d(save_dir: str, it: int, dynamic_syn: torch.Tensor, hal_weights: Sequence[torch.Tensor],
             hal_biases: Sequence[torch.Tensor], best: bool = False) -> None:
    """dynamic_syn (C,dpc,T,1,H,W); hallucinator i = (hal_weights[i], hal_biases[i])."""
    os.makedirs(save_dir, exist_ok=True)
    flat = dynamic_syn.detach().cpu().reshape((-1,) + tuple(dynamic_syn.shape[2:]))
    state: Dict[str, torch.Tensor] = {}
    for i, (w, b) in enumerate(zip(hal_weights, hal_biases)):
        state["%d.encoder.weight" % i] = w.detach().cpu()
        state["%d.encoder.bias" % i] = b.detach().cpu()
    torch.save(flat, os.path.join(save_dir, "dynamic_%d.pt" % it))
    torch.save(state, os.path.join(save_dir, "hal_%d.pt" % it))
    if best:
        torch.save(flat, os.path.join(save_dir, "dynamic_best.pt"))
        torch.save(state, os.path.join(save_dir, "weights_best.pt"))


def save_static(save_dir: str, it: int, static_syn: torch.Tensor, best: bool = False) -> str:
    """``static_{it}.pt`` / ``static_best.pt``: ``{"image": (C*spc,3,H,W)}``, row ``c*spc + j`` -- the file ``load_static`` and the
    reference's ``torch.load(path)["image"]`` read (``run_dc --memories static`` writes it)."""
    if static_syn.dim() != 4 or static_syn.shape[1] != 3:
        raise ValueError("save_static: a (C*spc, 3, H, W) tensor, not %s" % (tuple(static_syn.shape),))
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, "static_%d.pt" % it)
    blob = {"image": static_syn.detach().cpu().clone()}
    torch.save(blob, path)
    if best:
        torch.save(blob, os.path.join(save_dir, "static_best.pt"))
    return path


def load_static(path: str) -> torch.Tensor:
    """Static memory as the reference loads it: a dict with key "image" -> (C*spc,3,H,W)."""
    obj = torch.load(path, map_location="cpu")
    if not isinstance(obj, dict) or "image" not in obj:
        raise KeyError('static memory file must be a dict with key "image" (distill_s2d_ms.py:96-99)')
    return obj["image"].float()


def save_keyframes(save_dir: str, it: int, frames: torch.Tensor, interp: str, T: int, best: bool = False) -> str:
    """``keyframes_{it}.pt`` / ``keyframes_best.pt``: ``{"frames": (C*ipc,K,3,H,W) float32, "interp": str, "T": int}``, row
    ``c*ipc + j`` (``run_dm --memories keyframes`` writes it; this project's own format: the reference stores whole clips)."""
    from . import keyframes
    if frames.dim() != 5 or frames.shape[2] != 3:
        raise ValueError("save_keyframes: a (C*ipc, K, 3, H, W) tensor, not %s" % (tuple(frames.shape),))
    keyframes.table(int(T), int(frames.shape[1]), interp)          # (refuses a K / T / interp no table exists for)
    os.makedirs(save_dir, exist_ok=True)
    path = os.path.join(save_dir, "keyframes_%d.pt" % it)
    blob = {"frames": frames.detach().cpu().float().clone(), "interp": str(interp), "T": int(T)}
    torch.save(blob, path)
    if best:
        torch.save(blob, os.path.join(save_dir, "keyframes_best.pt"))
    return path


def load_keyframes(path: str):
    """-> (frames (C*ipc,K,3,H,W) float32, interp, T) of a ``keyframes_*.pt``."""
    obj = torch.load(path, map_location="cpu")
    if not isinstance(obj, dict) or not all(k in obj for k in ("frames", "interp", "T")):
        raise KeyError('a key-frame file is a dict with the keys "frames", "interp" and "T"')
    return obj["frames"].float(), str(obj["interp"]), int(obj["T"])


def keyframes_to_images(path: str) -> torch.Tensor:
    """The clips a ``keyframes_*.pt`` stands for, (C*ipc,T,3,H,W) float32 on the host -- what ``images_*.pt`` holds, so the
    result can be evaluated by the reference or be the init of ``run_mtt --memories images``.  The same products and adds, in
    the same order, as the device expansion."""
    from . import keyframes
    frames, interp, T = load_keyframes(path)
    return keyframes.expand_torch(frames, keyframes.table(T, int(frames.shape[1]), interp))


def load_hallucinators(path: str):
    """-> list of (weight, bias) from a ``hal_{it}.pt`` / ``weights_best.pt`` state dict."""
    state = torch.load(path, map_location="cpu")
    out, i = [], 0
    while "%d.encoder.weight" % i in state:
        out.append((state["%d.encoder.weight" % i], state["%d.encoder.bias" % i]))
        i += 1
    if not out:
        raise KeyError("no '{i}.encoder.weight' keys in %s" % path)
    return out


# ---- expert trajectories for MTT (buffer.py:75-104; distill_baseline.py:113-135, 203-216) -------
def save_expert_buffer(save_dir: str, trajectories) -> str:
    """``replay_buffer_{n}.pt``: list over experts of list over epochs of the 8 parameter tensors
    (CPU, parameters() order); n = first free index, as buffer.py:97-101."""
    os.makedirs(save_dir, exist_ok=True)
    n = 0
    while os.path.exists(os.path.join(save_dir, "replay_buffer_{}.pt".format(n))):
        n += 1
    path = os.path.join(save_dir, "replay_buffer_{}.pt".format(n))
    torch.save([[[p.detach().cpu() for p in ep] for ep in traj] for traj in trajectories], path)
    return path


def load_expert_buffers(buffer_dir: str, max_files: int = None):
    """All ``replay_buffer_*.pt`` of a directory, concatenated (distill_baseline.py:116-133);
    raises AssertionError like the reference when none is found."""
    files, n = [], 0
    while os.path.exists(os.path.join(buffer_dir, "replay_buffer_{}.pt".format(n))):
        files.append(os.path.join(buffer_dir, "replay_buffer_{}.pt".format(n)))
        n += 1
    if n == 0:
        raise AssertionError("No buffers detected at {}".format(buffer_dir))
    if max_files is not None:
        files = files[:max_files]
    out = []
    for f in files:
        out += torch.load(f, map_location="cpu")
    return out


def train_expert_trajectories(net_factory, trainloader, args, num_experts: int, train_epochs: int, lr_teacher: float = 0.01,
                              mom: float = 0.0, l2: float = 0.0, decay: bool = False):
    """The producer loop of buffer.py:64-95 (with ``args.eval_mode`` defined): every
    expert is a fresh network trained with SGD through ``utils.epoch('train')`` -- i.e. the HIP
    train step -- recording the parameters before training and after every epoch."""
    from . import utils
    criterion = torch.nn.CrossEntropyLoss().to(args.device)
    if not hasattr(args, "eval_mode"):
        args.eval_mode = "SS"
    trajectories = []
    for _ in range(num_experts):
        net = net_factory().to(args.device)
        net.train()
        lr = lr_teacher
        opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=mom, weight_decay=l2)
        stamps = [[p.detach().cpu() for p in net.parameters()]]
        for e in range(train_epochs):
            utils.epoch("train", trainloader, net, opt, criterion, args)
            stamps.append([p.detach().cpu() for p in net.parameters()])
            if decay and e == train_epochs // 2 + 1:
                lr *= 0.1
                opt = torch.optim.SGD(net.parameters(), lr=lr, momentum=mom, weight_decay=l2)
        trajectories.append(stamps)
    return trajectories
