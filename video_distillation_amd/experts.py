"""Expert trajectories for trajectory matching as flat rows: ``ExpertStore`` reads the ``replay_buffer_N.pt`` files of a
buffer directory (buffer.py / checkpoint.save_expert_buffer: a list over experts of lists over epochs of the 8 parameter
tensors) and hands ``MTTTrainer.step`` one expert at a time as a ``FlatTrajectory`` whose rows are 1-D fp32 DEVICE views in
``distill.flatten_params`` order -- the start and the target parameters of an iteration without 16 pageable host-to-device
copies and two ``torch.cat`` (distill_baseline.py:213-221).

Layout.  A file becomes one fp32 tensor (experts, epochs, Ppad); P = the 8 tensors' element count for ``num_classes``, Ppad = P
rounded up to a multiple of 4 floats (padding zero), so every row starts on a 16-byte boundary -- what the ``vdt_`` kernels of
include/vd_hip.h ask for (P is odd at 3 classes).

Modes.  ``resident``: every file the walk will use lives on the device from construction on; refused, before anything is
allocated there, when that is more than the device reports free.  ``host``: one file at a time in pinned host memory (a file is read, and its
epoch count compared with the files before it, when the walk reaches it); a row
that is asked for is copied into one of two device staging rows with ``non_blocking=True`` on the current stream, so an
iteration still enqueues without a host synchronisation.

Order.  It comes from ``random.Random(seed)`` alone, so every rank walks the same experts.  ``walk="all"`` is what the
reference's loop intends: shuffle the files; per file shuffle its experts and yield each; after the last file reshuffle the
files.  ``walk="reference"`` is what distill_baseline.py:203-211 and distill_s2d_ms.py:209-218 do: ``file_idx`` advances and
"loading file" is printed, but nothing is loaded again -- only the first file of the first shuffle is ever used, its experts
reshuffled at every wrap (the file list is reshuffled too when ``file_idx`` wraps, which moves the generator and nothing else).
"""
from __future__ import annotations

import os
import random
from typing import List, Optional

import numpy as np
import torch


def param_count(num_classes: int) -> int:
    from .distill import FULL_SHAPES
    return int(sum(int(np.prod(s)) for s in FULL_SHAPES(num_classes)))


def padded(p: int) -> int:
    return (int(p) + 3) // 4 * 4


def buffer_files(buffer_dir: str, max_files: Optional[int] = None) -> List[str]:
    """``replay_buffer_0.pt``, ``_1``, ... as checkpoint.load_expert_buffers finds them; AssertionError when there is none."""
    files, n = [], 0
    while os.path.exists(os.path.join(buffer_dir, "replay_buffer_{}.pt".format(n))):
        files.append(os.path.join(buffer_dir, "replay_buffer_{}.pt".format(n)))
        n += 1
    if n == 0:
        raise AssertionError("No buffers detected at {}".format(buffer_dir))
    return files if max_files is None else files[:int(max_files)]


def flatten_file(path: str, num_classes: int, pin: bool = False) -> torch.Tensor:
    """One buffer file -> (experts, epochs, Ppad) fp32 on the host, validated against ``FULL_SHAPES(num_classes)``."""
    from .distill import FULL_SHAPES
    shapes = [tuple(s) for s in FULL_SHAPES(num_classes)]
    P = param_count(num_classes)
    buf = torch.load(path, map_location="cpu")
    if not isinstance(buf, (list, tuple)) or not buf:
        raise ValueError("%s: expected a non-empty list of expert trajectories" % path)
    epochs = len(buf[0])
    for e, traj in enumerate(buf):
        if len(traj) != epochs:
            raise ValueError("%s: expert %d holds %d epochs, expert 0 holds %d -- the experts of a file have one length"
                             % (path, e, len(traj), epochs))
    out = torch.zeros((len(buf), epochs, padded(P)), dtype=torch.float32, pin_memory=pin)
    for e, traj in enumerate(buf):
        for t, params in enumerate(traj):
            got = int(sum(int(p.numel()) for p in params))
            if got != P or [tuple(p.shape) for p in params] != shapes:
                raise ValueError("%s: expert %d epoch %d holds %d parameters in %d tensors; --num_classes %d needs %d in %d "
                                 "(were the experts trained on another number of classes?)"
                                 % (path, e, t, got, len(params), num_classes, P, len(shapes)))
            o = 0
            for p in params:
                n = int(p.numel())
                out[e, t, o:o + n] = p.detach().reshape(-1).to(torch.float32)
                o += n
    return out


class FlatTrajectory:
    """One expert: ``row(epoch)`` -> 1-D fp32 device view of length P (16-byte aligned), ``epochs`` rows.  Of a ``host`` store's
    trajectory the two most recently requested rows are valid (two staging rows), and only until the store's next ``next()``."""

    def __init__(self, rows: torch.Tensor, P: int, staging: Optional[torch.Tensor] = None):
        self._rows, self.P, self.epochs = rows, int(P), int(rows.shape[0])
        self._staging = staging
        self._slot_of, self._next_slot = {}, 0

    def row(self, epoch: int) -> torch.Tensor:
        epoch = int(epoch)
        if not 0 <= epoch < self.epochs:
            raise IndexError("epoch %d of a trajectory of %d epochs" % (epoch, self.epochs))
        if self._staging is None:
            return self._rows[epoch, :self.P]
        slot = self._slot_of.get(epoch)
        if slot is None:
            slot = self._next_slot
            self._next_slot = (slot + 1) % int(self._staging.shape[0])
            self._slot_of = {e: s for e, s in self._slot_of.items() if s != slot}
            self._slot_of[epoch] = slot
            self._staging[slot].copy_(self._rows[epoch], non_blocking=True)          # pinned -> device on the current stream
        return self._staging[slot, :self.P]

    def __len__(self) -> int:
        return self.epochs


class ExpertStore:
    def __init__(self, buffer_dir: str, num_classes: int, device, mode: str = "host", walk: str = "all", seed: int = 0,
                 max_files: Optional[int] = None):
        if mode not in ("host", "resident"):
            raise ValueError("ExpertStore: mode %r (host or resident)" % (mode,))
        if walk not in ("all", "reference"):
            raise ValueError("ExpertStore: walk %r (all or reference)" % (walk,))
        self.device, self.mode, self.walk, self.num_classes = torch.device(device), mode, walk, int(num_classes)
        self.P = param_count(num_classes)
        self.Ppad = padded(self.P)
        self.files = buffer_files(buffer_dir, max_files)
        self._rng = random.Random(seed)
        self._order = list(range(len(self.files)))
        self._rng.shuffle(self._order)
        self._file_pos = 0
        used = self._order[:1] if walk == "reference" else sorted(self._order)
        self._pin = self.device.type == "cuda"
        self._dev = {}                    # resident mode: file number -> (experts, epochs, Ppad) on the device
        self.epochs = None
        if mode == "resident":
            # the files hold raw fp32 tensors and little else: their size on disk is the size of the rows (the padding to Ppad
            # adds less than 16 bytes a row).  The device is asked for nothing before the total is known to fit.
            need = sum(os.path.getsize(self.files[f]) for f in used)
            if self.device.type == "cuda":
                free, _ = torch.cuda.mem_get_info(self.device)
                if need > free:
                    raise RuntimeError("ExpertStore: the %d buffer file(s) of this walk hold %.2f GB of trajectories, the device "
                                       "reports %.2f GB free -- pass --max_files to use fewer files, or --expert_store host to "
                                       "keep one file at a time in pinned host memory" % (len(used), need / 1e9, free / 1e9))
            for f in used:          # one file on the host at a time
                t = flatten_file(self.files[f], self.num_classes)
                self._check_epochs(f, t)
                self._dev[f] = t.to(self.device)
                del t
            self._staging = None
        else:
            self._staging = torch.zeros((2, self.Ppad), dtype=torch.float32, device=self.device)
        self._load(self._order[0])

    def _check_epochs(self, f: int, t: torch.Tensor) -> None:
        if self.epochs is None:
            self.epochs = int(t.shape[1])
        elif int(t.shape[1]) != self.epochs:
            raise ValueError("%s holds %d epochs per expert, the files before it %d" % (self.files[f], int(t.shape[1]), self.epochs))

    def _load(self, f: int) -> None:
        """Make file ``f`` the current one and shuffle its experts."""
        if self.mode == "resident":
            self._cur = self._dev[f]
        else:
            # a fresh pinned block per file: the caching host allocator hands the previous one out again only after the
            # asynchronous copies that read it have finished
            self._cur = flatten_file(self.files[f], self.num_classes, pin=self._pin)
            self._check_epochs(f, self._cur)
        self.current_file = f
        self._experts = list(range(int(self._cur.shape[0])))
        self._rng.shuffle(self._experts)
        self._expert_pos = 0

    def check(self, max_start_epoch: int, expert_epochs: int) -> None:
        """Refuse, before the loop starts, settings whose target row does not exist (the reference raises IndexError at
        the first iteration that draws a late start epoch)."""
        last = int(max_start_epoch) - 1 + int(expert_epochs)
        if int(max_start_epoch) < 1 or int(expert_epochs) < 1 or last > self.epochs - 1:
            raise ValueError("--max_start_epoch %d --expert_epochs %d reads epoch %d of trajectories that hold epochs 0..%d "
                             "(%d rows per expert in %s)" % (max_start_epoch, expert_epochs, last, self.epochs - 1, self.epochs,
                                                            os.path.dirname(self.files[0])))

    def next(self) -> FlatTrajectory:
        if self._expert_pos == len(self._experts):          # the wrap of the previous call, done now: one file in memory at a time
            self._file_pos += 1
            if self._file_pos == len(self._order):
                self._file_pos = 0
                self._rng.shuffle(self._order)
            if self.walk == "all":
                self._load(self._order[self._file_pos])
            else:          # the reference never loads again: the same file, reshuffled
                self._rng.shuffle(self._experts)
                self._expert_pos = 0
        e = self._experts[self._expert_pos]
        self._expert_pos += 1
        self.last = (self.current_file, e)
        return FlatTrajectory(self._cur[e], self.P, self._staging)
