"""The C-ABI shared library loads and exports every symbol include/vd_hip.h declares, the binding takes every signature from
that header, and the ctypes struct mirrors and hand-mirrored constants have the layout and values the header gives them
(no compute calls: there is no GPU in the CPU test tier)."""
import ctypes
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"vd(?:t|s|sr)?_[a-z0-9_]+"          # vd_*, and the three historical prefixes of the sections at the header's end
PREFIXED = {"vdt_": ["vdt_traj_adjoint", "vdt_traj_loss", "vdt_traj_scratch_doubles", "vdt_traj_step"],
            "vds_": ["vds_still_expand", "vds_still_reduce"],
            "vdsr_": ["vdsr_still_rows"]}


def declared_functions():
    text = open(os.path.join(ROOT, "include", "vd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t|void|char\*)\s+(%s)\s*\(" % NAME, text)))


def test_header_and_binding_agree():
    from video_distillation_amd import hip
    assert declared_functions() == sorted(hip.EXPORTS)


def test_the_three_prefixed_sections_are_declared_bound_and_exported():
    """The exact name set of each historical prefix, in the header, in the binding and in the library; the other 86 are vd_*."""
    from video_distillation_amd import hip
    for prefix, names in PREFIXED.items():
        assert [n for n in declared_functions() if n.startswith(prefix)] == names == sorted(n for n in hip.EXPORTS if n.startswith(prefix))
    assert len([n for n in hip.EXPORTS if n.startswith("vd_")]) == 86 == len(hip.EXPORTS) - 7
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.bind(hip.LIB_PATH)
    for name in sum(PREFIXED.values(), []):
        assert hasattr(lib, name), name
    assert lib.vd_abi_version() == 5
    names = [os.path.basename(s) for s in hip.SOURCES]
    assert names[-1] == "traj.hip" and names[:2] == ["conv_mfma.hip", "aux_kernels.hip"]
    assert "still.hip" in names and "still_rows.hip" in names


def test_library_exports_every_declared_symbol():
    from video_distillation_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        hip.build()
    lib = hip.bind(hip.LIB_PATH)
    for name in declared_functions():
        assert hasattr(lib, name), name
    assert lib.vd_abi_version() == 5


def test_argument_errors_are_reported_before_any_device_call():
    """Entry points validate their arguments first (codes -1 / -2, include/vd_hip.h) -- callable without a GPU."""
    from video_distillation_amd import hip
    lib = hip.lib()
    assert lib.vd_conv_mfma(None, None) == -1
    assert lib.vd_conv_mfma_multi(None, 2, None) == -1
    a, b = hip.VdConvParams(), hip.VdConvParams()
    for p, mtw in ((a, 4), (b, 2)):        # two programs of different tile shapes do not share an instantiation
        p.prec, p.NT, p.MW, p.MTW, p.S, p.CC, p.ncl, p.lds_plane_bytes = 3, 1, 4, mtw, 8, 1, 1, 1024
    arr = (ctypes.POINTER(hip.VdConvParams) * 2)(ctypes.pointer(a), ctypes.pointer(b))
    assert lib.vd_conv_mfma_multi(arr, 0, None) == -1 and lib.vd_conv_mfma_multi(arr, 5, None) == -1
    assert lib.vd_conv_mfma_multi(arr, 2, None) == -2
    # a plain and an accumulating (atomic / select) program of the SAME tile shape do not share a launch either: the plain one
    # would run under the second-order instantiation (header: "all plain or all accumulating; -2 otherwise")
    c, d = hip.VdConvParams(), hip.VdConvParams()
    for p in (c, d):
        p.prec, p.NT, p.MW, p.MTW, p.S, p.CC, p.ncl, p.lds_plane_bytes = 2, 1, 4, 4, 8, 1, 1, 1024
    d.atomic = 1
    arr2 = (ctypes.POINTER(hip.VdConvParams) * 2)(ctypes.pointer(c), ctypes.pointer(d))
    assert lib.vd_conv_mfma_multi(arr2, 2, None) == -2
    d.atomic, d.select = 0, 1
    assert lib.vd_conv_mfma_multi(arr2, 2, None) == -2


def test_params_struct_layout_matches_header():
    """ctypes mirror of VdConvParams: same field order as the C struct (names must appear in the
    header in the same sequence); offsets and sizes: test_struct_mirrors_have_the_compiler_s_layout."""
    from video_distillation_amd import hip
    text = open(os.path.join(ROOT, "include", "vd_hip.h")).read()
    body = text[text.index("typedef struct VdConvParams {") + len("typedef struct VdConvParams {"):text.index("} VdConvParams;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl or decl.startswith("typedef"):
            continue
        decl = re.sub(r"^(const\s+)?[A-Za-z_0-9]+\s*\*?\s*", "", decl, count=1)
        names += [re.sub(r"\[.*\]", "", n.strip().lstrip("*")) for n in decl.split(",")]
    assert names == [f[0] for f in hip.VdConvParams._fields_]
    assert ctypes.sizeof(hip.VdConvParams) % 8 == 0


def _prototype_text():
    """include/vd_hip.h without comments, struct bodies and #define lines."""
    text = open(os.path.join(ROOT, "include", "vd_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"\{[^{}]*\}", "", text)
    return re.sub(r"^\s*#\s*define.*$", "", text, flags=re.M)


def test_every_prototype_of_the_header_is_parsed():
    from video_distillation_amd import hip
    assert len(hip.signatures()) == len(re.findall(r"\b%s\(" % NAME, _prototype_text())) == 93
    assert hip.EXPORTS == tuple(hip.signatures())
    defined = []
    csrc = os.path.join(ROOT, "video_distillation_amd", "csrc")
    for path in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.cpp")):
        defined += re.findall(r'extern\s+"C"\s+(?:const\s+)?\w+\s*\*?\s*(%s)\s*\(' % NAME, open(path).read())
    assert sorted(defined) == sorted(hip.signatures()) and len(defined) == 93


def test_signatures_pinned_by_hand():
    from video_distillation_amd import hip
    i, q, f, p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    pinned = {
        "vd_unpool_relu_bwd": (i, [p, p, q, i, i, i, i, i, i, i, i, i, p, p, i, p, p]),
        "vd_program_run": (i, [p, p, q, p, p, q, p, p, i, p]),
        "vd_sgd_momentum": (i, [p, p, p, q, f, f, i, p]),
        "vd_train_step": (i, [p, p, p, p, p, p, f, f, f, i, p, q, p, p, p]),
        "vd_conv_mfma_multi": (i, [p, i, p]),
        "vd_bias_grad_pooled_scratch_floats": (q, [q, i, q]),
        "vd_sources_hash": (ctypes.c_char_p, []),
        "vd_blob_free": (None, [p]),
    }
    assert len(pinned["vd_unpool_relu_bwd"][1]) == 17
    for name, want in pinned.items():
        assert hip.signatures()[name] == want, name
    lib = hip.lib()
    for name, (restype, argtypes) in hip.signatures().items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_signatures_of_the_prefixed_entry_points_pinned_by_hand():
    from video_distillation_amd import hip
    i, q, f, p = ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p
    pinned = {
        "vdt_traj_scratch_doubles": (q, [q]),
        "vdt_traj_step": (i, [p, p, p, q, p, p]),
        "vdt_traj_loss": (i, [p, p, p, q, p, p, p, p]),
        "vdt_traj_adjoint": (i, [p, p, p, p, f, q, p, p, p, p]),
        "vds_still_expand": (i, [p, p, q, i, i, i, p, p]),
        "vds_still_reduce": (i, [p, q, i, i, i, p, p]),
        "vdsr_still_rows": (i, [p, p, q, i, i, i, p, p, i, p]),
    }
    assert {name: sig for name, sig in hip.signatures().items() if not name.startswith("vd_")} == pinned          # all seven
    lib = hip.lib()
    for name, (restype, argtypes) in pinned.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        lib.vdt_traj_step(None, None, None, 4, None)           # a wrong count is an exception before the call


@pytest.mark.parametrize("text,quoted", [
    ("int vd_a(int n);\nint vd_b(float* x, unsigned long n, void* stream);\n", "unsigned long n"),
    ("int vd_a(int n);\nint vd_b(void (*done)(int), void* stream);\n", "void (*done)(int)"),
    ("int vd_a(int n);\nint vd_b(const float* x, int64_t n,\n", "vd_b(const float* x, int64_t n,"),
    ("int vd_a(uint8_t flag);\n", "uint8_t flag"),
    ("float vd_a(int n);\n", "float vd_a(int n)"),
    ("int vd_a(int n);\nint vd_a(int64_t n);\n", "int vd_a(int64_t n)"),
])
def test_the_parser_refuses_what_it_does_not_know(text, quoted):
    from video_distillation_amd import hip
    with pytest.raises(ValueError) as e:
        hip.parse_header("/* a header */\n#include <stdint.h>\n" + text)
    assert quoted in str(e.value)


@pytest.mark.parametrize("prefix", ["vdt_", "vds_", "vdsr_"])
def test_the_parser_names_the_header_it_refuses(prefix):
    from video_distillation_amd import hip
    with pytest.raises(ValueError, match=r"^include/vd_hip\.h: .*unsigned n"):
        hip.parse_header("int %sa(unsigned n);" % prefix)
    with pytest.raises(ValueError, match=r"^some/other\.h: "):
        hip.parse_header("int %sa(unsigned n);" % prefix, "some/other.h")


def test_plain_python_ints_travel_in_the_declared_width():
    from video_distillation_amd import hip
    assert hip.lib().vd_bias_grad_pooled_scratch_floats(2 ** 33, 8, 256) == 2 ** 36


def test_wrong_arguments_are_exceptions_before_the_call():
    from video_distillation_amd import hip
    lib = hip.lib()
    with pytest.raises(TypeError):
        lib.vd_bias_grad_pooled_scratch_floats(2, 8)
    with pytest.raises(TypeError):
        lib.vd_bias_grad_pooled_scratch_floats(2, 8, 256, 0)
    with pytest.raises(ctypes.ArgumentError):
        lib.vd_group_sum(None, 1, 1, 1, ctypes.c_double(1.0), None, None)           # a double into `float scale`
    with pytest.raises(ctypes.ArgumentError):
        lib.vd_bias_grad_pooled_scratch_floats(2, ctypes.c_int64(8), 256)           # 64 bits into `int C`
    with pytest.raises(RuntimeError, match=r"^vd_conv_mfma\(level0\) failed with code -1$"):
        hip.run("vd_conv_mfma", None, None, what="vd_conv_mfma(level0)")
    with pytest.raises(RuntimeError, match=r"^vd_conv_mfma failed with code -1$"):
        hip.run("vd_conv_mfma", None, None)


def _mirror_fields(struct):
    return [(name, getattr(struct, name).offset, getattr(struct, name).size) for name, *_ in struct._fields_]


def test_struct_mirrors_have_the_compiler_s_layout(tmp_path):
    """A host program compiled from the header prints sizeof of the five structs the binding mirrors and offsetof / size of
    every field the mirrors name; the ctypes layout must be the same, and so must the two array bounds."""
    from video_distillation_amd import hip
    structs = [hip.VdConvParams, hip.VdMatchSeg, hip.VdMatchBatch, hip.VdPackSeg, hip.VdPackBatch]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "vd_hip.h"', 'int main() {',
             '    std::printf("VD_PACK_MAX %d\\nVD_MATCH_MAX_SEG %d\\n", VD_PACK_MAX, VD_MATCH_MAX_SEG);']
    for s in structs:
        n = s.__name__
        lines.append('    std::printf("%s %%zu\\n", sizeof(%s));' % (n, n))
        for f, _, _ in _mirror_fields(s):
            lines.append('    std::printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (n, f, n, f, n, f))
    lines += ['    return 0;', '}']
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(line.split(None, 1) for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {"VD_PACK_MAX": "%d" % hip.VD_PACK_MAX, "VD_MATCH_MAX_SEG": "%d" % hip.VD_MATCH_MAX_SEG}
    for s in structs:
        want[s.__name__] = "%d" % ctypes.sizeof(s)
        for f, offset, size in _mirror_fields(s):
            want["%s.%s" % (s.__name__, f)] = "%d %d" % (offset, size)
    assert got == want


def test_product_has_no_cpu_fallback():
    import torch
    from video_distillation_amd import networks, utils
    net = networks.ConvNet3D(3, 5, 128, 3, 'relu', 'none', 'maxpooling', 8, (64, 64))
    with pytest.raises(RuntimeError):
        net.embed(torch.zeros(1, 8, 3, 64, 64))
    with pytest.raises(RuntimeError):
        utils.Conv3DNet()(torch.zeros(1, 3, 8, 8), torch.zeros(1, 2, 1, 8, 8))
    # nothing under the product package imports the oracle
    pkg = os.path.join(ROOT, "video_distillation_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_library_carries_the_hash_of_its_sources_and_a_stale_one_is_refused(tmp_path, monkeypatch):
    """Round 6: the library is stamped with the sha256 of the kernel sources + header it was built from (csrc/stamp.cpp);
    ``hip.build`` / ``hip.lib`` decide staleness by that stamp, not by mtimes -- a library built from touched sources is
    rebuilt, and refused when it cannot be."""
    import shutil
    import subprocess
    from video_distillation_amd import hip
    hip.build()
    want = hip.sources_hash()
    assert hip.library_stamp() == want and len(want) == 16
    lib = hip.bind(hip.LIB_PATH)
    assert lib.vd_sources_hash().decode() == hip.STAMP_PREFIX + want
    # a copy of the library next to "touched" sources (one byte appended to a copy of a kernel file): the stamp no longer matches
    stale = tmp_path / "libvd_hip.so"
    shutil.copy(hip.LIB_PATH, stale)
    src = tmp_path / "aux_kernels.hip"
    shutil.copy(hip.SOURCES[1], src)
    with open(src, "a") as f:
        f.write("\n// touched\n")
    monkeypatch.setattr(hip, "SOURCES", [hip.SOURCES[0], str(src)] + hip.SOURCES[2:])
    monkeypatch.setattr(hip, "LIB_PATH", str(stale))
    monkeypatch.setattr(hip, "_lib", None)
    assert hip.sources_hash() != want and hip.library_stamp(str(stale)) == want

    def no_compiler(*a, **k):
        raise subprocess.CalledProcessError(127, "hipcc")
    monkeypatch.setattr(hip, "build", no_compiler)
    with pytest.raises(RuntimeError, match="built from other sources"):
        hip.lib()


def test_sources_hash_covers_the_header_the_kernel_files_and_the_shared_headers(tmp_path, monkeypatch):
    from video_distillation_amd import hip
    want = hip.sources_hash()
    other = tmp_path / "vd_hip.h"
    other.write_text(open(hip.HEADER).read() + "\n/* touched */\n")
    monkeypatch.setattr(hip, "HEADER", str(other))
    assert hip.sources_hash() != want
    monkeypatch.undo()
    assert hip.sources_hash() == want
    for name, attr in (("still.hip", "SOURCES"), ("still_rows.hip", "SOURCES"), ("split16.h", "CSRC_HEADERS")):
        paths = getattr(hip, attr)
        src = tmp_path / name
        src.write_text(open([s for s in paths if s.endswith("/" + name)][0]).read() + "\n// touched\n")
        monkeypatch.setattr(hip, attr, [str(src) if s.endswith("/" + name) else s for s in paths])
        assert hip.sources_hash() != want, name
        monkeypatch.undo()


def test_constants_mirrored_by_hand_equal_the_header_s_defines():
    """hip.py reads no file on import, so it restates a few of the header's ``#define``s; each is compared here."""
    import inspect
    from video_distillation_amd import hip
    text = re.sub(r"/\*.*?\*/", "", open(hip.HEADER).read(), flags=re.S)
    defines = {name: int(value) for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VD_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)}
    assert hip.PREC == {name[len("VD_PREC_"):].lower(): v for name, v in defines.items() if name.startswith("VD_PREC_")}
    assert len(hip.PREC) == 5 and sorted(hip.PREC.values()) == [0, 1, 2, 3, 4]
    assert hip.F16X3_WSHIFT == defines["VD_F16X3_WSHIFT"]
    assert hip.VD_PACK_MAX == defines["VD_PACK_MAX"] and hip.VD_MATCH_MAX_SEG == defines["VD_MATCH_MAX_SEG"]
    assert hip.CORESET_METHOD == {"herding": defines["VD_CORESET_HERDING"], "k-center": defines["VD_CORESET_KCENTER"]}
    assert defines["VD_ABI_VERSION"] == 5
    assert "vd_abi_version() != %d:" % defines["VD_ABI_VERSION"] in inspect.getsource(hip.lib)
