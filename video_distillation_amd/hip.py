"""ctypes binding of libvd_hip.so.  The headers of ``HEADERS`` (include/vd_hip.h first) are the one declaration of its C ABI: every
entry point's ``restype`` and ``argtypes`` are parsed from them (``bind``), call sites pass plain Python values, a wrong count or
type raises before the call.

PyTorch is used only as the owner of device memory and streams: every call passes
``tensor.data_ptr()`` and the current HIP stream handle.  There is deliberately NO fallback:
if the shared library is missing or a kernel launch fails, a RuntimeError is raised.
"""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvd_hip.so")
SOURCES = [os.path.join(_HERE, "csrc", f) for f in ("conv_mfma.hip", "aux_kernels.hip", "program.hip", "planner.cpp", "comm.cpp",
                                                         "coreset.hip", "clips_sample.hip", "eval_stats.hip", "regress_stats.hip", "still.hip", "still_rows.hip",
                                                         "nfr.hip", "frepo.hip", "keyframes.hip", "traj.hip")]
CSRC_HEADERS = [os.path.join(_HERE, "csrc", f) for f in ("frame_norm.h", "split16.h")]      # included by more than one source: part of every hash below
STAMP_SOURCE = os.path.join(_HERE, "csrc", "stamp.cpp")      # vd_sources_hash(): compiled on every link with the hash of SOURCES + header
INCLUDE = os.path.join(_HERE, "..", "include")
NAME_PATTERN = r"vd(?:t|s|sr)?_[a-z0-9_]+"          # include/vd_hip.h: vd_* and its three historical prefixes
# The C ABI: (file under INCLUDE -- an absolute path stands for itself --, the pattern its function names match in full).  Parsing (``signatures``), binding
# (``all_signatures``) and both hashes (``header_paths``) read this table and nothing else; a new header is one row here.
HEADERS = (("vd_hip.h", NAME_PATTERN),
           ("vd_keyframes.h", r"vdk_[a-z0-9_]+"),      # csrc/keyframes.hip
           ("vd_nfr.h", r"vdn_[a-z0-9_]+"),      # csrc/nfr.hip
           ("vd_frepo.h", r"vdf_[a-z0-9_]+"),      # csrc/frepo.hip
           ("vd_regress.h", r"vdr_[a-z0-9_]+"))      # csrc/regress_stats.hip

CORESET_METHOD = {"herding": 0, "k-center": 1}      # include/vd_hip.h VD_CORESET_HERDING / VD_CORESET_KCENTER
PREC = {"bf16": 0, "f16": 1, "bf16x3": 2, "f16x3": 3, "f16c8": 4}      # f16c8: fp16 + fp8 corrections (the real side's last level only)
F16X3_WSHIFT = 8          # include/vd_hip.h VD_F16X3_WSHIFT: packed fp16 hi+lo weights are W x 2^8, undone in the programs' epilogues
# include/vd_hip.h VD_PERSIST_*: VdConvParams.persist = box-walk generations (low 16 bits) | the options of single programs
PERSIST_GENS_MASK = 0xFFFF
PERSIST_PLAIN_K = 1 << 19       # vd_conv0_breg: the plain K loop on a frame-tile program
PERSIST_NO_ALT = 1 << 20        # hi+lo programs: no per-chunk sign alternation of the accumulation


class VdConvParams(ctypes.Structure):
    _fields_ = [
        ("src", ctypes.c_void_p), ("src_plane_stride4", ctypes.c_int64),
        ("src_clip_stride4", ctypes.c_int64), ("src_chunk_stride4", ctypes.c_int64),
        ("wpk", ctypes.c_void_p), ("w_plane_stride", ctypes.c_int64), ("w_box_stride", ctypes.c_int64),
        ("bias", ctypes.c_void_p),
        ("dst", ctypes.c_void_p), ("dst_plane_stride", ctypes.c_int64),
        ("argmax", ctypes.c_void_p), ("col_off", ctypes.c_void_p), ("out_scale", ctypes.c_void_p),
        ("type_desc", ctypes.c_void_p), ("tables", ctypes.c_void_p), ("boxes", ctypes.c_void_p),
        ("gather", ctypes.c_void_p), ("gather_stride", ctypes.c_int64), ("zero_slot", ctypes.c_void_p),
        ("nbox", ctypes.c_int32), ("nclips", ctypes.c_int32), ("ncl", ctypes.c_int32),
        ("CC", ctypes.c_int32), ("S", ctypes.c_int32), ("NT", ctypes.c_int32), ("MW", ctypes.c_int32), ("MTW", ctypes.c_int32),
        ("epi", ctypes.c_int32), ("pool_t", ctypes.c_int32), ("relu", ctypes.c_int32),
        ("n_out", ctypes.c_int32), ("n_stride", ctypes.c_int32),
        ("out_clip_stride", ctypes.c_int64),
        ("out_chunk_stride", ctypes.c_int32), ("out_t_stride", ctypes.c_int32),
        ("lds_plane_bytes", ctypes.c_int32), ("prec", ctypes.c_int32), ("dbg", ctypes.c_int32), ("ntypes", ctypes.c_int32), ("tab_ofs", ctypes.c_int32 * 3), ("atomic", ctypes.c_int32), ("select", ctypes.c_int32), ("src_split_cc", ctypes.c_int32), ("src_split_off4", ctypes.c_int64), ("NTW", ctypes.c_int32), ("clip_index", ctypes.c_void_p), ("mt_valid", ctypes.c_int32), ("persist", ctypes.c_int32), ("stamps", ctypes.c_void_p),
        ("w_set_clips", ctypes.c_int32), ("replica_stride", ctypes.c_int32), ("emit_lo", ctypes.c_int32), ("src_planes", ctypes.c_int32), ("src_rows", ctypes.c_int32), ("pair_flip", ctypes.c_int32), ("range_stats", ctypes.c_void_p),
    ]


class VdMatchSeg(ctypes.Structure):
    _fields_ = [("gr", ctypes.c_void_p), ("gs", ctypes.c_void_p), ("g", ctypes.c_void_p), ("rows", ctypes.c_int64),
                ("len", ctypes.c_int32), ("reserved", ctypes.c_int32)]


VD_PACK_MAX = 24


class VdPackSeg(ctypes.Structure):
    _fields_ = [("w", ctypes.c_void_p), ("widx", ctypes.c_void_p), ("n", ctypes.c_int64), ("out_hi", ctypes.c_void_p),
                ("out_lo", ctypes.c_void_p), ("prec", ctypes.c_int32), ("first_block", ctypes.c_int32)]


class VdPackBatch(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seg", VdPackSeg * VD_PACK_MAX)]


VD_MATCH_MAX_SEG = 16


class VdMatchBatch(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int32), ("reserved", ctypes.c_int32), ("seg", VdMatchSeg * VD_MATCH_MAX_SEG)]


def build(force: bool = False, verbose: bool = False, debug_hooks: bool = False) -> str:
    """Compile the HIP sources for gfx950 into libvd_hip.so (in-tree).  ``debug_hooks`` builds the
    variant libvd_hip_dbg.so with the ablation / timing hooks of VdConvParams.dbg compiled in
    (-DVD_DBG_HOOKS=1; used by tools/ablate.py and tools/stamps.py via VD_LIB_VARIANT=dbg).

    Staleness is decided by CONTENT, not by mtime (round 6): the library carries the sha256 of the sources it was built from
    (csrc/stamp.cpp, ``vd_sources_hash``) and is rebuilt when that differs from ``sources_hash()`` of this checkout; every
    object file has a side file with the hash of its source + the header."""
    out = LIB_PATH.replace(".so", "_dbg.so") if debug_hooks else LIB_PATH
    if not force and library_stamp(out) == sources_hash():
        return out
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # one object per source (rebuilt only when that source or the header changed), compiled concurrently, then one link
    objdir = os.path.join(_HERE, "csrc", "build_dbg" if debug_hooks else "build")
    os.makedirs(objdir, exist_ok=True)
    # one builder at a time (several ranks / test workers may find the library stale together): an exclusive lock on the object
    # directory; whoever waited finds the library fresh and returns
    import fcntl
    lock = open(os.path.join(objdir, ".lock"), "w")
    fcntl.flock(lock, fcntl.LOCK_EX)
    try:
        return _build_locked(out, objdir, hipcc, force, verbose, debug_hooks)
    finally:
        fcntl.flock(lock, fcntl.LOCK_UN)
        lock.close()


def _file_hash(*paths: str) -> str:
    import hashlib
    h = hashlib.sha256()
    for path in paths:
        with open(path, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def header_paths() -> list:
    """The headers of ``HEADERS`` in table order (resolved per call: a test may replace the table)."""
    return [os.path.join(INCLUDE, name) for name, _ in HEADERS]


def _object_key(src: str) -> str:
    """What one source's object file is stamped with: the source, every ABI header and the shared csrc headers."""
    return _file_hash(src, *header_paths(), *CSRC_HEADERS)


def _build_locked(out: str, objdir: str, hipcc: str, force: bool, verbose: bool, debug_hooks: bool) -> str:
    want = sources_hash()
    if not force and library_stamp(out) == want:
        return out
    flags = ["-O3", "--offload-arch=gfx950", "-fPIC"] + (["-DVD_DBG_HOOKS=1"] if debug_hooks else [])
    jobs, objs = [], []
    for src in SOURCES:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        side = obj + ".srchash"
        objs.append(obj)
        key = _object_key(src)
        have = open(side).read().strip() if os.path.exists(side) and os.path.exists(obj) else None
        if force or have != key:
            if os.path.exists(side):
                os.remove(side)
            cmd = [hipcc] + flags + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd), side, key))
    for cmd, pr, side, key in jobs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
        with open(side, "w") as f:
            f.write(key)
    stamp_obj = os.path.join(objdir, "stamp.cpp.o")
    cmd = [hipcc, "-O2", "-fPIC", "-DVD_SOURCES_HASH=\"%s%s\"" % (STAMP_PREFIX, want), "-c", STAMP_SOURCE, "-o", stamp_obj]
    subprocess.run(cmd, check=True)
    tmp = out + ".tmp.%d" % os.getpid()       # (linked beside the target and renamed: a reader never maps a half-written library)
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp] + objs + [stamp_obj, "-ldl"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    return out


STAMP_PREFIX = "VD_SOURCES_HASH="


def library_stamp(path: str = None) -> Optional[str]:
    """The sources hash a built library carries (read from the file's bytes, no dlopen: a stale library must not be mapped into
    the process that is about to rebuild it), or None if the file is missing or unstamped."""
    path = path or LIB_PATH
    if not os.path.exists(path):
        return None
    import mmap
    with open(path, "rb") as f:
        with mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
            i = m.find(STAMP_PREFIX.encode())
            if i < 0:
                return None
            return m[i + len(STAMP_PREFIX):i + len(STAMP_PREFIX) + 16].decode("ascii", "replace")


def sources_hash() -> str:
    """sha256 (first 16 hex digits) over the kernel sources, the ABI header and the shared csrc headers: what measurement files
    that are carried from one run to the next (profiles/rNN_pmc_traffic.json -> bench.py's ``roofline.traffic``) are stamped
    with, so that a figure measured on other kernels is refused instead of quoted."""
    return _file_hash(*sorted(SOURCES), *header_paths(), *CSRC_HEADERS)


_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "int64_t": ctypes.c_int64, "float": ctypes.c_float, "double": ctypes.c_double}
_RETURNS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "void": None, "const char*": ctypes.c_char_p}
_PROTOTYPE = r"(int64_t|int|void|const char\s*\*)\s*(%s)\s*\(([^()]*)\)"
_PARAMETER = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\b\s*)?)*)\b\w+")


def parse_header(text: str, where: str = "include/vd_hip.h", names: str = NAME_PATTERN) -> dict:
    """The prototypes of a C header in the closed set of spellings include/vd_hip.h uses -> {name: (restype, [argtypes])}.
    ``names``: the regular expression a function name has to match in full (default: ``vd_*`` and the three historical prefixes
    ``vdt_*``, ``vds_*``, ``vdsr_*``).  Anything else -- another name, a type outside the set, a statement that is not wholly a
    prototype -- is a ``ValueError`` that names ``where`` and quotes it; no guesses."""
    prototype = re.compile(_PROTOTYPE % names)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"typedef\s+struct\s*\w*\s*(\{[^{}]*\}\s*)?\w+\s*;", " ", text)
    text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{|^[ \t]*\}[ \t]*$', " ", text, flags=re.M)      # (no directive is continued)
    sigs = {}
    for stmt in filter(None, (" ".join(part.split()) for part in text.split(";"))):
        m = prototype.fullmatch(stmt)
        if m is None or m.group(2) in sigs:
            raise ValueError("%s: not a prototype the binding understands, or a second one of its name: %r" % (where, stmt))
        ret, name, params = m.group(1).replace(" *", "*"), m.group(2), m.group(3).strip()
        argtypes = []
        for par in ([] if params == "void" else params.split(",")):
            pm = _PARAMETER.fullmatch(par.strip())
            if pm is None or not (pm.group(2) or pm.group(1) in _SCALARS):
                raise ValueError("%s: parameter %r of %r has no ctypes mapping" % (where, par.strip(), stmt))
            argtypes.append(ctypes.c_void_p if pm.group(2) else _SCALARS[pm.group(1)])
        sigs[name] = (_RETURNS[ret], argtypes)
    return sigs


@functools.lru_cache(maxsize=None)
def signatures(header: str = "vd_hip.h") -> dict:
    """{name: (restype, [argtypes])} of one header of ``HEADERS`` (default: include/vd_hip.h, the 93 names of ``EXPORTS``), read
    and parsed with its own name pattern once, when first asked for (binding a library does).  ``KeyError`` for another header."""
    names = dict(HEADERS)[header]
    with open(os.path.join(INCLUDE, header)) as f:
        return parse_header(f.read(), "include/" + os.path.basename(header), names)


def all_signatures() -> dict:
    """The signatures of every header of ``HEADERS``, in table order: what ``bind`` sets and a built library has to export."""
    merged, owner = {}, {}
    for header, _ in HEADERS:
        for name, sig in signatures(header).items():
            if name in merged:
                raise ValueError("%s is declared by %s and by %s" % (name, owner[name], header))
            merged[name], owner[name] = sig, header
    return merged


def __getattr__(name: str):          # hip.EXPORTS: the header's names, without reading it at import
    if name == "EXPORTS":
        return tuple(signatures())
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


class _Library(ctypes.CDLL):
    # ctypes lets a cdecl function take MORE arguments than its argtypes (C varargs); without FUNCFLAG_CDECL the count has to be
    # exact, and the flag selects another calling convention on 32-bit Windows only.  That is how CPython reads the flag, not
    # documented behaviour: tests/test_cabi.py::test_wrong_arguments_are_exceptions_before_the_call guards it
    _func_flags_ = 0


def bind(path: str, allow_missing: bool = False) -> ctypes.CDLL:
    """Open the library at ``path`` with every entry point's ``restype`` / ``argtypes`` set from the headers of ``HEADERS``."""
    L = _Library(path)
    for name, (restype, argtypes) in all_signatures().items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        elif not allow_missing:
            raise RuntimeError("libvd_hip.so does not export %s" % name)
    return L


_lib: Optional[ctypes.CDLL] = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        path = os.environ.get("VD_LIB_PATH", LIB_PATH)           # (measurement tools: A/B of two builds on one box)
        if os.environ.get("VD_LIB_VARIANT") == "dbg":      # profiling tools: the build with the dbg hooks compiled in
            path = build(debug_hooks=True)
        if not os.path.exists(path):
            raise RuntimeError(
                "libvd_hip.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU or eager fallback for the HIP path)" % path)
        if "VD_LIB_PATH" not in os.environ and os.environ.get("VD_LIB_VARIANT") != "dbg":
            # the numbers of a run come from THIS file: it must be the build of this checkout's kernel sources (the stamp
            # compiled into it, not its mtime, says so).  A stale library is rebuilt when a compiler is there, refused otherwise.
            want = sources_hash()
            if library_stamp(path) != want:
                try:
                    build()
                except (OSError, subprocess.CalledProcessError) as e:
                    raise RuntimeError("libvd_hip.so at %s was built from other sources (stamp %s, checkout %s) and could not be "
                                       "rebuilt: %s" % (path, library_stamp(path), want, e))
                if library_stamp(path) != want:
                    raise RuntimeError("libvd_hip.so at %s carries stamp %s, the checkout's kernel sources hash to %s"
                                       % (path, library_stamp(path), want))
        L = bind(path, allow_missing="VD_LIB_PATH" in os.environ)      # (an older build loaded on purpose for an A/B measurement)
        if L.vd_abi_version() != 5:
            raise RuntimeError("libvd_hip.so ABI version mismatch")
        _lib = L
    return _lib


def loaded_stamp() -> str:
    """Sources hash compiled into the library this process runs on (bench.py and smoke() print it)."""
    v = lib().vd_sources_hash().decode()
    return v[len(STAMP_PREFIX):] if v.startswith(STAMP_PREFIX) else v


def deterministic() -> bool:
    """Whether accumulations run in a fixed order (bitwise reproducible training step): the library's process-wide
    switch, initialised from VD_DETERMINISTIC."""
    return bool(lib().vd_get_deterministic())


def set_deterministic(on: bool) -> bool:
    """Switch the fixed-order accumulation mode; engines / programs created afterwards follow it.  Returns the previous value."""
    return bool(lib().vd_set_deterministic(int(bool(on))))


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def check(code: int, what: str) -> None:
    if code != 0:
        raise RuntimeError("%s failed with code %d" % (what, code))


def run(name: str, *args, what: Optional[str] = None) -> None:
    """Call entry point ``name`` and raise on a non-zero code (``what``: its name in the message where that says more)."""
    check(getattr(lib(), name)(*args), what or name)


def ptr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def is_x3(prec: int) -> bool:
    return prec >= 2


EVAL_STATS_HEAD = 8          # include/vd_hip.h vd_eval_stats: scalar slots in front of the two per-class blocks


def eval_stats_record(num_classes: int, device=None) -> torch.Tensor:
    """A zeroed record for ``eval_stats``: 8 + 2K doubles (layout: include/vd_hip.h)."""
    return torch.zeros(EVAL_STATS_HEAD + 2 * int(num_classes), dtype=torch.float64, device=device)


def eval_stats(logits: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor) -> torch.Tensor:
    """Accumulate the test statistics of one batch -- clips, cross-entropy sum, top-1/3/5 hits, labels out of range, hits and
    clips per class -- into ``rec`` (vd_eval_stats, one launch on the current stream).  Device tensors always go to the kernel;
    CPU tensors take the same definitions in torch fp64 (as utils._standardize does for CPU tensors: the host logic of
    evalpool.py then runs under gloo without a GPU)."""
    if logits.dim() != 2:
        raise ValueError("eval_stats: logits (B, K)")
    B, K = int(logits.shape[0]), int(logits.shape[1])
    if K < 1 or tuple(labels.shape) != (B,) or rec.dtype != torch.float64 or rec.numel() != EVAL_STATS_HEAD + 2 * K \
            or not rec.is_contiguous():
        raise ValueError("eval_stats: logits (B, K), labels (B,), rec %d contiguous doubles" % (EVAL_STATS_HEAD + 2 * K))
    if logits.device != labels.device or logits.device != rec.device:
        raise ValueError("eval_stats: logits, labels and rec live on one device")
    z = logits.detach().to(torch.float32).contiguous()
    y = labels.detach().to(torch.int64).contiguous()
    if z.is_cuda:
        run("vd_eval_stats", ptr(z), ptr(y), B, K, ptr(rec), stream_ptr(z.device))
        return rec
    if B == 0:
        return rec
    valid = (y >= 0) & (y < K)
    rec[5] += float((~valid).sum())
    z, y = z[valid].double(), y[valid]
    if y.numel() == 0:
        return rec
    zy = z.gather(1, y[:, None])
    index = torch.arange(K)[None, :]
    rank = ((z > zy) | ((z == zy) & (index < y[:, None]))).sum(1)
    m = z.max(dim=1, keepdim=True).values
    ce = (m + torch.log(torch.exp(z - m).sum(1, keepdim=True)) - zy)[:, 0]
    rec[0] += float(y.numel())
    rec[1] += ce.sum()
    for slot, k in ((2, 1), (3, 3), (4, 5)):
        rec[slot] += float((rank < k).sum())
    rec[EVAL_STATS_HEAD:EVAL_STATS_HEAD + K] += torch.bincount(y[rank < 1], minlength=K).double()
    rec[EVAL_STATS_HEAD + K:] += torch.bincount(y, minlength=K).double()
    return rec


def regress_stats(logits: torch.Tensor, labels: torch.Tensor, rec: torch.Tensor) -> torch.Tensor:
    """Accumulate the regression test statistics of one batch -- clips, the sum of squared errors against ``frepo.soft_labels``
    (``one_hot - 1 / K`` in fp32), top-1/3/5 hits, labels out of range, hits and clips per class -- into ``rec``, a record of
    ``eval_stats_record`` (vdr_regress_stats, one launch on the current stream; layout: include/vd_regress.h).  ``labels`` are
    the integer labels.  Device tensors always go to the kernel; CPU tensors take the same definitions in torch fp64, as
    ``eval_stats`` does, so that the host logic of evalpool.py runs under gloo without a GPU."""
    if logits.dim() != 2:
        raise ValueError("regress_stats: logits (B, K)")
    B, K = int(logits.shape[0]), int(logits.shape[1])
    if K < 1 or tuple(labels.shape) != (B,) or labels.is_floating_point() or rec.dtype != torch.float64 \
            or rec.numel() != EVAL_STATS_HEAD + 2 * K or not rec.is_contiguous():
        raise ValueError("regress_stats: logits (B, K), integer labels (B,), rec %d contiguous doubles" % (EVAL_STATS_HEAD + 2 * K))
    if logits.device != labels.device or logits.device != rec.device:
        raise ValueError("regress_stats: logits, labels and rec live on one device")
    z = logits.detach().to(torch.float32).contiguous()
    y = labels.detach().to(torch.int64).contiguous()
    if z.is_cuda:
        with torch.cuda.device(z.device):
            run("vdr_regress_stats", ptr(z), ptr(y), B, K, ptr(rec), stream_ptr(z.device))
        return rec
    if B == 0:
        return rec
    valid = (y >= 0) & (y < K)
    rec[5] += float((~valid).sum())
    z, y = z[valid], y[valid]
    if y.numel() == 0:
        return rec
    soft = (torch.nn.functional.one_hot(y, num_classes=K) - 1 / K).float()      # (frepo.soft_labels, which imports this module)
    zy = z.gather(1, y[:, None])
    index = torch.arange(K)[None, :]
    rank = ((z > zy) | ((z == zy) & (index < y[:, None]))).sum(1)
    rec[0] += float(y.numel())
    rec[1] += ((z.double() - soft.double()) ** 2).sum()
    for slot, k in ((2, 1), (3, 3), (4, 5)):
        rec[slot] += float((rank < k).sum())
    rec[EVAL_STATS_HEAD:EVAL_STATS_HEAD + K] += torch.bincount(y[rank < 1], minlength=K).double()
    rec[EVAL_STATS_HEAD + K:] += torch.bincount(y, minlength=K).double()
    return rec


def check_hallucinator_tables(ns: int, nd: int, nh: int, sidx, didx, hidx):
    """Host-side bounds check of the index tables of one ``vd_hallucinator_fwd_multi`` call -> (sidx int64, didx int64,
    hidx int32) as contiguous numpy arrays of one length.  ``ValueError`` for anything the kernel must not be handed (it does
    not check its indices)."""
    import numpy as np
    s = np.ascontiguousarray(np.asarray(sidx, dtype=np.int64).reshape(-1))
    d = np.ascontiguousarray(np.asarray(didx, dtype=np.int64).reshape(-1))
    h = np.ascontiguousarray(np.asarray(hidx, dtype=np.int64).reshape(-1))
    if not s.size == d.size == h.size:
        raise ValueError("hallucinator tables: %d static, %d dynamic and %d hallucinator indices" % (s.size, d.size, h.size))
    for name, t, hi in (("sidx", s, ns), ("didx", d, nd), ("hidx", h, nh)):
        if t.size and (t.min() < 0 or t.max() >= hi):
            raise ValueError("hallucinator tables: %s %d is outside [0, %d)" % (name, int(t[(t < 0) | (t >= hi)][0]), hi))
    return s, d, h.astype(np.int32)


def hallucinate_multi(static: torch.Tensor, dynamic: torch.Tensor, sidx, didx, hidx, weights: torch.Tensor, biases: torch.Tensor,
                      extra=None):
    """``vd_hallucinator_fwd_multi`` on the current stream: out[i] = hallucinator ``hidx[i]`` over (static[sidx[i]],
    dynamic[didx[i]]).  ``static`` (ns, 3, H, W), ``dynamic`` (nd, T, 1, H, W), ``weights`` (nh, 3, 4, 3, 3, 3) and ``biases``
    (nh, 3) are contiguous fp32 tensors on one device; ``sidx`` / ``didx`` / ``hidx`` are HOST tables of one length n.
    -> a fresh (n, T, 3, H, W) fp32 tensor, or (that, the device copy of ``extra``) when ``extra`` -- an int64 host array of
    n entries that rides in the same upload, e.g. the batch's labels -- is given.

    The tables are validated here, on the host (``ValueError``: an index out of range never reaches the device), packed into
    ONE pinned buffer and uploaded with one asynchronous copy; nothing synchronises."""
    import numpy as np
    if static.dim() != 4 or dynamic.dim() != 5 or static.shape[1] != 3 or dynamic.shape[2] != 1 \
            or tuple(static.shape[2:]) != tuple(dynamic.shape[3:]):
        raise ValueError("hallucinate_multi: static (ns, 3, H, W) and dynamic (nd, T, 1, H, W)")
    nh = int(weights.shape[0]) if weights.dim() == 6 else 0
    if nh < 1 or tuple(weights.shape[1:]) != (3, 4, 3, 3, 3) or tuple(biases.shape) != (nh, 3):
        raise ValueError("hallucinate_multi: weights (nh, 3, 4, 3, 3, 3) and biases (nh, 3)")
    s, d, h = check_hallucinator_tables(int(static.shape[0]), int(dynamic.shape[0]), nh, sidx, didx, hidx)
    n, (T, H, W) = s.size, (int(dynamic.shape[1]), int(dynamic.shape[3]), int(dynamic.shape[4]))
    if n > 65535:
        raise ValueError("hallucinate_multi: %d clips in one launch (at most 65535)" % n)
    e = None if extra is None else np.asarray(extra, dtype=np.int64).reshape(-1)
    if e is not None and e.size != n:
        raise ValueError("hallucinate_multi: extra holds %d entries for %d clips" % (e.size, n))
    for t in (static, dynamic, weights, biases):
        if not (t.is_cuda and t.device == dynamic.device and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("hallucinate_multi has no CPU path: contiguous fp32 tensors on one HIP device")
    dev = dynamic.device
    out = torch.empty((n, T, 3, H, W), dtype=torch.float32, device=dev)
    ne = 0 if e is None else n
    if n == 0:
        return out if e is None else (out, torch.as_tensor(e).to(dev))
    # one pinned buffer: sidx (int64) | didx (int64) | extra (int64) | hidx (int32).  A fresh pinned block per call: the
    # caching host allocator hands it out again only after the copy below has finished.
    o_d, o_e, o_h = 8 * n, 16 * n, 16 * n + 8 * ne
    host = torch.empty((o_h + 4 * n,), dtype=torch.uint8).pin_memory()
    hv = host.numpy()
    hv[:o_d].view(np.int64)[:] = s
    hv[o_d:o_e].view(np.int64)[:] = d
    if ne:
        hv[o_e:o_h].view(np.int64)[:] = e
    hv[o_h:].view(np.int32)[:] = h
    tab = host.to(dev, non_blocking=True)
    base = tab.data_ptr()
    with torch.cuda.device(dev):
        run("vd_hallucinator_fwd_multi", ptr(static), ptr(dynamic), base, base + o_d, base + o_h, ptr(weights), ptr(biases), nh, n,
            T, H, W, ptr(out), stream_ptr(dev))
    return out if e is None else (out, tab[o_e:o_h].view(torch.int64))


def _still_tensor(t: torch.Tensor, dims: int, what: str) -> None:
    if t.dim() != dims or int(t.shape[-3]) != 3:
        raise ValueError("%s: a (%s3, H, W) tensor, not %s" % (what, "n, " if dims == 4 else "n, T, ", tuple(t.shape)))
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError("%s has no CPU path: a contiguous fp32 tensor on a HIP device" % what)


def _still_index(index, N: int, dev, what: str, checked: bool = False):
    """``index`` of a still wrapper -> (n, its int64 table of n rows on ``dev``), (N, None) for None.  A HOST table (array, list,
    CPU tensor) is checked here and uploaded with one copy, a device tensor is checked with one device reduction (a host read)
    unless the caller says it has ``checked`` it.  ``ValueError`` for a row outside [0, N)."""
    import numpy as np
    if index is None:
        return N, None
    if isinstance(index, torch.Tensor) and index.is_cuda:
        idx = index.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        bad = bool(((idx < 0) | (idx >= N)).any()) if idx.numel() and not checked else False
    else:
        host = np.ascontiguousarray(np.asarray(index, dtype=np.int64).reshape(-1))
        bad = bool(host.size) and (int(host.min()) < 0 or int(host.max()) >= N)
        idx = None if bad else torch.as_tensor(host).to(dev)
    if bad:
        raise ValueError("%s: an index outside [0, %d)" % (what, N))
    return int(idx.numel()), idx


def still_expand(images: torch.Tensor, index, T: int, checked: bool = False) -> torch.Tensor:
    """``vds_still_expand`` on the current stream: -> a fresh (n, T, 3, H, W) tensor, out[i, t] = images[index[i]] (``index``
    None: out[i, t] = images[i]).  ``images`` (N, 3, H, W) contiguous fp32 on a HIP device.  ``index`` may repeat rows; a host
    table or a device tensor, checked as ``_still_index`` says (``checked``: a device tensor the caller has checked).
    ``ValueError`` for a row outside [0, N): it never reaches the kernel, which does not check."""
    _still_tensor(images, 4, "still_expand: images")
    N, H, W, T = int(images.shape[0]), int(images.shape[2]), int(images.shape[3]), int(T)
    if T < 1 or H < 1 or W < 1:
        raise ValueError("still_expand: T %d, H %d, W %d" % (T, H, W))
    dev = images.device
    n, idx = _still_index(index, N, dev, "still_expand", checked)
    out = torch.empty((n, T, 3, H, W), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        run("vds_still_expand", ptr(images), ptr(idx), n, T, H, W, ptr(out), stream_ptr(dev))
    return out


def still_rows(images: torch.Tensor, index, T: int, prec: int, planes: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``vdsr_still_rows`` on the current stream: the first-level operand rows of the still clips ``images[index]`` repeated over
    ``T`` frames, -> (planes, n * T * 3 * H * pitch / 8, 8) int16 (``out``: that tensor, or a larger contiguous one of ``planes``
    planes whose leading part is written), byte for byte ``vd_pix2rows`` of ``still_expand(images, index, T)``.  ``prec`` one of
    the four codes ``PREC['bf16'] .. PREC['f16x3']`` (0..3); ``planes`` 2 also writes the low plane.  ``index`` is
    validated as ``still_expand`` validates it: ``ValueError`` for a row outside [0, N) before anything reaches the kernel."""
    if images.dim() != 4 or int(images.shape[1]) != 3:
        raise ValueError("still_rows: images: a (n, 3, H, W) tensor, not %s" % (tuple(images.shape),))
    N, H, W, T = int(images.shape[0]), int(images.shape[2]), int(images.shape[3]), int(T)
    if T < 1 or H < 1 or W < 1 or prec not in (0, 1, 2, 3) or planes not in (1, 2):
        raise ValueError("still_rows: T %d, H %d, W %d, prec %r, planes %r" % (T, H, W, prec, planes))
    dev = images.device
    n, idx = _still_index(index, N, dev, "still_rows")      # (a bad table is refused before the device of ``images`` is looked at)
    _still_tensor(images, 4, "still_rows: images")
    slots = n * T * 3 * H * ((W + 8 + 7) // 8)
    if out is None:
        out = torch.empty((planes, slots, 8), dtype=torch.int16, device=dev)
    elif not (out.is_cuda and out.device == dev and out.dtype == torch.int16 and out.dim() == 3 and out.is_contiguous()
              and int(out.shape[0]) == planes and int(out.shape[1]) >= slots and int(out.shape[2]) == 8):
        raise ValueError("still_rows: out is a contiguous (%d, >= %d, 8) int16 tensor on %s" % (planes, slots, dev))
    with torch.cuda.device(dev):
        run("vdsr_still_rows", ptr(images), ptr(idx), n, T, H, W, ptr(out[0]), ptr(out[1] if planes == 2 else None), int(prec),
            stream_ptr(dev))
    return out


def still_reduce(g_clips: torch.Tensor) -> torch.Tensor:
    """``vds_still_reduce`` on the current stream: (n, T, 3, H, W) -> a fresh (n, 3, H, W) tensor, the sum over the frames in
    ascending t, one fp32 add per frame (bitwise repeatable)."""
    _still_tensor(g_clips, 5, "still_reduce: g_clips")
    n, T, _, H, W = (int(v) for v in g_clips.shape)
    if T < 1 or H < 1 or W < 1:
        raise ValueError("still_reduce: T %d, H %d, W %d" % (T, H, W))
    out = torch.empty((n, 3, H, W), dtype=torch.float32, device=g_clips.device)
    with torch.cuda.device(g_clips.device):
        run("vds_still_reduce", ptr(g_clips), n, T, H, W, ptr(out), stream_ptr(g_clips.device))
    return out


VDK_MAX_FRAMES = 64          # include/vd_keyframes.h


class VdkTable(ctypes.Structure):
    _fields_ = [("T", ctypes.c_int32), ("K", ctypes.c_int32), ("i0", ctypes.c_int32 * VDK_MAX_FRAMES), ("i1", ctypes.c_int32 * VDK_MAX_FRAMES),
                ("w0", ctypes.c_float * VDK_MAX_FRAMES), ("w1", ctypes.c_float * VDK_MAX_FRAMES)]


def vdk_table(table) -> VdkTable:
    """The ctypes mirror of a ``keyframes.Table`` (anything with ``T``, ``K`` and the four length-T arrays): host memory, passed
    by address; the library copies it into the kernel arguments.  ``ValueError`` for what ``vdk_table_check`` would refuse."""
    if isinstance(table, VdkTable):
        return table
    if getattr(table, "_vdk", None) is not None:          # (a keyframes.Table keeps its mirror: built and checked once, not per step)
        return table._vdk
    T, K = int(table.T), int(table.K)
    if not (1 <= K <= T <= VDK_MAX_FRAMES) or any(len(a) != T for a in (table.i0, table.i1, table.w0, table.w1)):
        raise ValueError("key-frame table: T %d, K %d, arrays of %s entries" % (T, K, [len(a) for a in (table.i0, table.i1, table.w0, table.w1)]))
    c = VdkTable()
    c.T, c.K = T, K
    for t in range(T):
        c.i0[t], c.i1[t], c.w0[t], c.w1[t] = int(table.i0[t]), int(table.i1[t]), float(table.w0[t]), float(table.w1[t])
    if lib().vdk_table_check(ctypes.addressof(c)) != 0:
        raise ValueError("key-frame table: an index outside [0, %d) or a weight that is not finite" % K)
    if hasattr(table, "_vdk"):
        table._vdk = c
    return c


def _keyframe_tensor(t: torch.Tensor, frames: int, what: str) -> None:
    if t.dim() != 5 or int(t.shape[1]) != frames or int(t.shape[2]) != 3 or int(t.shape[3]) < 1 or int(t.shape[4]) < 1:
        raise ValueError("%s: a (n, %d, 3, H, W) tensor, not %s" % (what, frames, tuple(t.shape)))
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise RuntimeError("%s has no CPU path: a contiguous fp32 tensor on a HIP device" % what)


def keyframe_expand(keys: torch.Tensor, table) -> torch.Tensor:
    """``vdk_keyframe_expand`` on the current stream: (n, K, 3, H, W) -> a fresh (n, T, 3, H, W) tensor, frame t =
    w0[t] * key i0[t] + w1[t] * key i1[t] (``table``: a ``keyframes.Table`` or a ``VdkTable``).  ``keys`` contiguous fp32 on a
    HIP device; shapes and the table are checked here, on the host."""
    tab = vdk_table(table)
    _keyframe_tensor(keys, tab.K, "keyframe_expand: keys")
    n, _, _, H, W = (int(v) for v in keys.shape)
    out = torch.empty((n, tab.T, 3, H, W), dtype=torch.float32, device=keys.device)
    with torch.cuda.device(keys.device):
        run("vdk_keyframe_expand", ptr(keys), n, ctypes.addressof(tab), H, W, ptr(out), stream_ptr(keys.device))
    return out


def keyframe_reduce(g_clips: torch.Tensor, table) -> torch.Tensor:
    """``vdk_keyframe_reduce`` on the current stream: (n, T, 3, H, W) -> a fresh (n, K, 3, H, W) tensor, the adjoint of
    ``keyframe_expand``: per key the products w * g[t] of its terms, added in ascending t (bitwise repeatable)."""
    tab = vdk_table(table)
    _keyframe_tensor(g_clips, tab.T, "keyframe_reduce: g_clips")
    n, _, _, H, W = (int(v) for v in g_clips.shape)
    out = torch.empty((n, tab.K, 3, H, W), dtype=torch.float32, device=g_clips.device)
    with torch.cuda.device(g_clips.device):
        run("vdk_keyframe_reduce", ptr(g_clips), n, ctypes.addressof(tab), H, W, ptr(out), stream_ptr(g_clips.device))
    return out


VDN_MAX_SYN = 1024          # include/vd_nfr.h
VDN_LDS_SYN = 128


def _nfr_dims(feat_syn: torch.Tensor, feat_tar: torch.Tensor, labels: torch.Tensor, label_rows: str, what: str):
    """Shapes, then dtypes and devices of one kernel-ridge call -> (n, m, d, c); ``labels`` is (n, c) or (m, c) (``label_rows``).
    ``ValueError`` for shapes that do not fit or dimensions the op refuses, ``RuntimeError`` for what is not a contiguous fp32
    tensor on a HIP device."""
    label_name = "y_syn" if label_rows == "n" else "g_pred"
    if feat_syn.dim() != 2 or feat_tar.dim() != 2 or labels.dim() != 2 or feat_tar.shape[1] != feat_syn.shape[1] \
            or labels.shape[0] != (feat_syn.shape[0] if label_rows == "n" else feat_tar.shape[0]):
        raise ValueError("%s: feat_syn (n, d), feat_tar (m, d) and %s (%s, c), not %s, %s and %s"
                         % (what, label_name, label_rows, tuple(feat_syn.shape), tuple(feat_tar.shape), tuple(labels.shape)))
    n, d, m, c = int(feat_syn.shape[0]), int(feat_syn.shape[1]), int(feat_tar.shape[0]), int(labels.shape[1])
    if not (1 <= n <= VDN_MAX_SYN and m >= 1 and d >= 1 and c >= 1):
        raise ValueError("%s: n %d (1..%d), m %d, d %d, c %d" % (what, n, VDN_MAX_SYN, m, d, c))
    for name, t in (("feat_syn", feat_syn), ("feat_tar", feat_tar), (label_name, labels)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
            raise RuntimeError("%s: %s has no CPU path: a contiguous fp32 tensor on a HIP device" % (what, name))
        if t.device != feat_syn.device:
            raise ValueError("%s: the tensors live on one device" % what)
    return n, m, d, c


def nfr_forward(feat_syn: torch.Tensor, y_syn: torch.Tensor, feat_tar: torch.Tensor, reg: float = 1e-6):
    """``vdn_nfr_forward`` on the current stream: the kernel ridge predictor of include/vd_nfr.h.  ``feat_syn`` (n, d), ``y_syn``
    (n, c), ``feat_tar`` (m, d): contiguous fp32 on one HIP device.  -> (pred (m, c) fp64, workspace): the workspace, allocated
    here, is what ``nfr_backward`` and ``nfr_status`` take.  Nothing synchronises with the host."""
    n, m, d, c = _nfr_dims(feat_syn, feat_tar, y_syn, "n", "nfr_forward")
    dev = feat_syn.device
    nbytes = int(lib().vdn_nfr_workspace_bytes(n, m, d, c))
    if nbytes < 0:
        raise ValueError("nfr_forward: dimensions (%d, %d, %d, %d) are refused" % (n, m, d, c))
    workspace = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    pred = torch.empty((m, c), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        run("vdn_nfr_forward", ptr(feat_syn), ptr(y_syn), ptr(feat_tar), n, m, d, c, float(reg), ptr(workspace), ptr(pred), stream_ptr(dev))
    return pred, workspace


def nfr_backward(feat_syn: torch.Tensor, feat_tar: torch.Tensor, g_pred: torch.Tensor, workspace: torch.Tensor, reg: float = 1e-6):
    """``vdn_nfr_backward`` on the current stream, from the workspace of the ``nfr_forward`` call with the same features and
    ``reg``: ``g_pred`` (m, c) contiguous fp32 -> (g_feat_syn (n, d), g_y_syn (n, c)), both fp64.  The workspace is only read."""
    n, m, d, c = _nfr_dims(feat_syn, feat_tar, g_pred, "m", "nfr_backward")
    dev = feat_syn.device
    if not (workspace.is_cuda and workspace.device == dev and workspace.dtype == torch.float64 and workspace.is_contiguous()
            and workspace.numel() * 8 == int(lib().vdn_nfr_workspace_bytes(n, m, d, c))):
        raise ValueError("nfr_backward: the workspace is not that of a forward call with these dimensions on %s" % dev)
    g_feat = torch.empty((n, d), dtype=torch.float64, device=dev)
    g_y = torch.empty((n, c), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        run("vdn_nfr_backward", ptr(feat_syn), ptr(feat_tar), ptr(g_pred), n, m, d, c, float(reg), ptr(workspace), ptr(g_feat), ptr(g_y),
            stream_ptr(dev))
    return g_feat, g_y


def nfr_status(workspace: torch.Tensor) -> int:
    """The status word of a workspace (a host read: it waits for the forward call): 0, or k + 1 when pivot k was the first that
    was not positive and finite."""
    return int(workspace[:1].view(torch.int64).item())


VDF_ADAM_MAX = 16          # include/vd_frepo.h


class VdfAdamSeg(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("g", ctypes.c_void_p), ("n", ctypes.c_int64),
                ("step_size", ctypes.c_float), ("lr_wd", ctypes.c_float), ("first_block", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class VdfAdamBatch(ctypes.Structure):
    _fields_ = [("nseg", ctypes.c_int32), ("reserved", ctypes.c_int32), ("beta1", ctypes.c_float), ("one_minus_beta1", ctypes.c_float),
                ("beta2", ctypes.c_float), ("one_minus_beta2", ctypes.c_float), ("bc2_sqrt", ctypes.c_float), ("eps", ctypes.c_float),
                ("seg", VdfAdamSeg * VDF_ADAM_MAX)]


def mse_loss(logits: torch.Tensor, targets: torch.Tensor):
    """``vdf_mse_loss`` on the current stream: ``nn.MSELoss()`` of ``logits`` (B, K) against ``targets`` (B, K), both contiguous
    fp32 on one HIP device -> (loss: a fresh device scalar, dlogits (B, K))."""
    if logits.dim() != 2 or tuple(targets.shape) != tuple(logits.shape) or logits.numel() == 0:
        raise ValueError("mse_loss: logits (B, K) and targets (B, K), not %s and %s" % (tuple(logits.shape), tuple(targets.shape)))
    for name, t in (("logits", logits), ("targets", targets)):
        if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.device == logits.device):
            raise RuntimeError("mse_loss: %s has no CPU path: a contiguous fp32 tensor on one HIP device" % name)
    B, K = int(logits.shape[0]), int(logits.shape[1])
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dlog = torch.empty((B, K), dtype=torch.float32, device=logits.device)
    with torch.cuda.device(logits.device):
        run("vdf_mse_loss", ptr(logits), ptr(targets), B, K, ptr(loss), ptr(dlog), stream_ptr(logits.device))
    return loss, dlog


def adam_constants(lr: float, beta1: float, beta2: float, step: int):
    """(step_size, bc2_sqrt) of step ``step`` >= 1 in double, exactly as ``torch.optim.Adam`` computes them
    (``lr / (1 - beta1 ** step)``, ``(1 - beta2 ** step) ** 0.5``); the launch rounds each to float once."""
    return float(lr) / (1.0 - float(beta1) ** int(step)), (1.0 - float(beta2) ** int(step)) ** 0.5


def adam_multi(segments, beta1: float, beta2: float, eps: float, step: int) -> None:
    """``vdf_adam_multi`` on the current stream: one Adam / AdamW step ``step`` (>= 1, shared) over ``segments``, a sequence of
    ``(p, m, v, g, lr, weight_decay)`` -- four fp32 device tensors of one element count, contiguous (views at any float offset
    are fine), updated in place but for ``g``; ``weight_decay`` is AdamW's decoupled decay (0: Adam).  One launch per
    ``VDF_ADAM_MAX`` segments."""
    segments = list(segments)
    if int(step) < 1:
        raise ValueError("adam_multi: step %r (the count after the increment, >= 1)" % (step,))
    if not segments:
        return
    dev = segments[0][0].device
    for p, m, v, g, _, _ in segments:
        for name, t in (("p", p), ("m", m), ("v", v), ("g", g)):
            if not (t.is_cuda and t.device == dev and t.dtype == torch.float32 and t.is_contiguous()):
                raise RuntimeError("adam_multi: %s has no CPU path: contiguous fp32 tensors on one HIP device" % name)
            if t.numel() != p.numel() or t.numel() < 1:
                raise ValueError("adam_multi: p, m, v and g hold %s elements" % ([x.numel() for x in (p, m, v, g)],))
    st = stream_ptr(dev)
    with torch.cuda.device(dev):
        for lo in range(0, len(segments), VDF_ADAM_MAX):
            part = segments[lo:lo + VDF_ADAM_MAX]
            b = VdfAdamBatch()
            b.nseg = len(part)
            b.beta1, b.one_minus_beta1, b.beta2, b.one_minus_beta2 = beta1, 1.0 - beta1, beta2, 1.0 - beta2
            b.eps = eps
            b.bc2_sqrt = adam_constants(0.0, beta1, beta2, step)[1]
            for k, (p, m, v, g, lr, wd) in enumerate(part):
                s = b.seg[k]
                s.p, s.m, s.v, s.g, s.n = ptr(p), ptr(m), ptr(v), ptr(g), p.numel()
                s.step_size, s.lr_wd = adam_constants(lr, beta1, beta2, step)[0], float(lr) * float(wd)
            run("vdf_adam_multi", ctypes.addressof(b), st)


class Comm:
    """An RCCL communicator behind the C ABI (vd_comm_*, include/vd_hip.h): created over the ranks of the default torch.distributed
    group (rank 0's 128-byte id travels through ``broadcast_object_list``), collectives issued on the caller's CURRENT HIP stream.
    Used where the exchange goes through the library's own entry points instead of torch's process group (bench.py's
    ``--exchange allreduce`` leg and the rccl block of its JSON line)."""

    def __init__(self, rank: int, world: int):
        import torch.distributed as dist
        ident = (ctypes.c_char * 128)()
        if rank == 0:
            run("vd_comm_unique_id", ident)
        if world > 1:
            box = [bytes(ident)]
            dist.broadcast_object_list(box, src=0)
            ident = (ctypes.c_char * 128).from_buffer_copy(box[0])
        self._c = ctypes.c_void_p()
        run("vd_comm_create", ident, world, rank, ctypes.byref(self._c))
        self.rank, self.world = rank, world

    def size(self) -> int:
        return int(lib().vd_comm_size(self._c))

    @staticmethod
    def version() -> Optional[int]:
        v = ctypes.c_int(0)
        return int(v.value) if lib().vd_comm_version(ctypes.byref(v)) == 0 else None

    def all_reduce(self, t: torch.Tensor) -> None:
        assert t.dtype == torch.float32 and t.is_contiguous()
        run("vd_comm_allreduce_f32", self._c, ptr(t), ptr(t), t.numel(), stream_ptr(t.device))

    def free(self) -> None:
        if self._c:
            lib().vd_comm_free(self._c)
            self._c = ctypes.c_void_p()
