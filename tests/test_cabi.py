"""The C-ABI shared library loads and exports every symbol the headers of ``hip.HEADERS`` declare, the binding takes every signature
from those headers, both hashes cover them, and the ctypes struct mirrors and hand-mirrored constants have the layout and values
the headers give them (no compute calls: there is no GPU in the CPU test tier).

A new header is one row of ``hip.HEADERS``, one row of ``ABI`` and one dict of ``PINNED`` here, and one row of ``LAYOUTS`` if it
has structs."""
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
# header -> (the prefix of its names, their pattern, how many it declares, the one source that defines them all); the test's own
# copy of hip.HEADERS, in its order
ABI = {"vd_hip.h": ("vd_", NAME, 93, None),
       "vd_keyframes.h": ("vdk_", r"vdk_[a-z0-9_]+", 3, "keyframes.hip"),
       "vd_nfr.h": ("vdn_", r"vdn_[a-z0-9_]+", 3, "nfr.hip"),
       "vd_frepo.h": ("vdf_", r"vdf_[a-z0-9_]+", 2, "frepo.hip"),
       "vd_regress.h": ("vdr_", r"vdr_[a-z0-9_]+", 1, "regress_stats.hip")}
SOURCES = ["conv_mfma.hip", "aux_kernels.hip", "program.hip", "planner.cpp", "comm.cpp", "coreset.hip", "clips_sample.hip", "eval_stats.hip",
           "regress_stats.hip", "still.hip", "still_rows.hip", "nfr.hip", "frepo.hip", "keyframes.hip", "traj.hip"]          # hip.SOURCES: the link order
_i, _q, _f, _d, _p =ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
# signatures pinned by hand: every name of the four newer headers and all seven prefixed ones of vd_hip.h, eight of its vd_*
PINNED = {
    "vd_hip.h": {
        "vd_unpool_relu_bwd": (_i, [_p, _p, _q, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p, _p]),
        "vd_program_run": (_i, [_p, _p, _q, _p, _p, _q, _p, _p, _i, _p]),
        "vd_sgd_momentum": (_i, [_p, _p, _p, _q, _f, _f, _i, _p]),
        "vd_train_step": (_i, [_p, _p, _p, _p, _p, _p, _f, _f, _f, _i, _p, _q, _p, _p, _p]),
        "vd_conv_mfma_multi": (_i, [_p, _i, _p]),
        "vd_bias_grad_pooled_scratch_floats": (_q, [_q, _i, _q]),
        "vd_sources_hash": (ctypes.c_char_p, []),
        "vd_blob_free": (None, [_p]),
        "vdt_traj_scratch_doubles": (_q, [_q]),
        "vdt_traj_step": (_i, [_p, _p, _p, _q, _p, _p]),
        "vdt_traj_loss": (_i, [_p, _p, _p, _q, _p, _p, _p, _p]),
        "vdt_traj_adjoint": (_i, [_p, _p, _p, _p, _f, _q, _p, _p, _p, _p]),
        "vds_still_expand": (_i, [_p, _p, _q, _i, _i, _i, _p, _p]),
        "vds_still_reduce": (_i, [_p, _q, _i, _i, _i, _p, _p]),
        "vdsr_still_rows": (_i, [_p, _p, _q, _i, _i, _i, _p, _p, _i, _p]),
    },
    "vd_keyframes.h": {
        "vdk_table_check": (_i, [_p]),
        "vdk_keyframe_expand": (_i, [_p, _q, _p, _i, _i, _p, _p]),
        "vdk_keyframe_reduce": (_i, [_p, _q, _p, _i, _i, _p, _p]),
    },
    "vd_nfr.h": {
        "vdn_nfr_workspace_bytes": (_q, [_i, _i, _i, _i]),
        "vdn_nfr_forward": (_i, [_p, _p, _p, _i, _i, _i, _i, _d, _p, _p, _p]),
        "vdn_nfr_backward": (_i, [_p, _p, _p, _i, _i, _i, _i, _d, _p, _p, _p, _p]),
    },
    "vd_frepo.h": {"vdf_mse_loss": (_i, [_p, _p, _i, _i, _p, _p, _p]), "vdf_adam_multi": (_i, [_p, _p])},
    "vd_regress.h": {"vdr_regress_stats": (_i, [_p, _p, _i, _i, _p, _p])},
}


def declared_functions(header="vd_hip.h"):
    """The names ``header`` declares, by a regular expression of the test's own over the text without comments."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(?:int|int64_t|void|char\*)\s+(%s)\s*\(" % ABI[header][1], text)))


def _bound():
    from video_distillation_amd import hip
    return hip.bind(hip.LIB_PATH if os.path.exists(hip.LIB_PATH) else hip.build())


def test_the_headers_table_is_the_one_the_tests_cover():
    from video_distillation_amd import hip
    assert tuple((h, names) for h, (_, names, _, _) in ABI.items()) == tuple(hip.HEADERS) and list(PINNED) == list(ABI)
    assert [os.path.normpath(p) for p in hip.header_paths()] == [os.path.join(ROOT, "include", h) for h in ABI]
    assert len(hip.signatures()) == 93 == len(hip.EXPORTS) and hip.EXPORTS == tuple(hip.signatures("vd_hip.h"))
    others = tuple(prefix for prefix, *_ in list(ABI.values())[1:])
    assert not any(n.startswith(others) for n in hip.EXPORTS)          # vd_hip.h stays closed: no name of another header's prefix
    merged = hip.all_signatures()
    assert len(merged) == 93 + 3 + 3 + 2 + 1 and list(merged) == [n for h in ABI for n in hip.signatures(h)]
    for unknown in ("vd_other.h", "include/vd_hip.h", ""):
        with pytest.raises((KeyError, ValueError), match=re.escape(repr(unknown))):
            hip.signatures(unknown)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "for name in hip.all_signatures():" in entry          # build() checks every header's exports


def test_a_name_declared_by_two_headers_is_refused(tmp_path, monkeypatch):
    from video_distillation_amd import hip
    (tmp_path / "vd_twice.h").write_text("int vdk_table_check(const void* table);\n")
    monkeypatch.setattr(hip, "HEADERS", hip.HEADERS + ((str(tmp_path / "vd_twice.h"), ABI["vd_keyframes.h"][1]),))
    with pytest.raises(ValueError, match=r"vdk_table_check.*vd_keyframes\.h.*vd_twice\.h"):
        hip.all_signatures()


@pytest.mark.parametrize("header", list(ABI))
def test_names_are_declared_parsed_pinned_bound_exported_and_defined(header):
    """Per header the same name set five ways: the test's regular expression over the text, ``hip.signatures(header)``, the pinned
    dict (with the signatures), a bound library (``restype`` / ``argtypes``; a bound name is an exported one) and, where one
    source defines the header, that source's ``extern "C"`` definitions."""
    from video_distillation_amd import hip
    prefix, names, count, source = ABI[header]
    sigs = hip.signatures(header)
    assert sorted(sigs) == declared_functions(header) and len(sigs) == count
    assert {n: sigs[n] for n in PINNED[header]} == PINNED[header]
    assert {n: s for n, s in sigs.items() if not n.startswith("vd_")} == {n: s for n, s in PINNED[header].items() if not n.startswith("vd_")}
    lib = _bound()
    for name, (restype, argtypes) in sigs.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert lib.vd_abi_version() == 5
    if source is not None:
        text = open(os.path.join(ROOT, "video_distillation_amd", "csrc", source)).read()
        assert sorted(re.findall(r'extern\s+"C"\s+\w+\s+(%s)\s*\(' % names, text)) == sorted(sigs)


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
    assert [os.path.basename(s) for s in hip.SOURCES] == SOURCES and len(SOURCES) == 15


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
    header in the same sequence); offsets and sizes: test_mirrors_have_the_layout_the_compiler_gives_the_header."""
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
    """The library the process runs on (``hip.lib()``) carries the signatures of every header, the pinned ones among them."""
    from video_distillation_amd import hip
    assert len(PINNED["vd_hip.h"]["vd_unpool_relu_bwd"][1]) == 17
    lib = hip.lib()
    for header, pinned in PINNED.items():
        for name, (restype, argtypes) in list(pinned.items()) + list(hip.signatures(header).items()):
            fn = getattr(lib, name)
            assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_signatures_of_the_prefixed_entry_points_pinned_by_hand():
    from video_distillation_amd import hip
    pinned = {name: sig for name, sig in PINNED["vd_hip.h"].items() if not name.startswith("vd_")}
    assert len(pinned) == 7 and sorted(pinned) == sorted(sum(PREFIXED.values(), []))
    assert {name: sig for name, sig in hip.signatures().items() if not name.startswith("vd_")} == pinned          # all seven
    lib = hip.lib()
    with pytest.raises(TypeError):
        lib.vdt_traj_step(None, None, None, 4, None)           # a wrong count is an exception before the call
    with pytest.raises(TypeError):
        lib.vdk_keyframe_expand(None, 1, None, 5, 7, None)          # under another header's table as well


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


@pytest.mark.parametrize("header", list(ABI))
def test_each_header_s_pattern_refuses_the_other_headers_names(header):
    """The name pattern is an argument of the parser: under a header's own pattern its prefix parses, every other header's prefix
    and every other header's text is a ``ValueError`` that starts with the ``where`` it was given."""
    from video_distillation_amd import hip
    where, names = "include/" + header, dict(hip.HEADERS)[header]
    assert hip.parse_header("int %sa(int n);" % ABI[header][0], where, names) == {ABI[header][0] + "a": (_i, [_i])}
    for other in ABI:
        if other != header:
            with pytest.raises(ValueError, match="^" + re.escape(where) + ": "):
                hip.parse_header("int %sa(int n);" % ABI[other][0], where, names)
            with pytest.raises(ValueError, match="^" + re.escape(where) + ": "):
                hip.parse_header(open(os.path.join(ROOT, "include", other)).read(), where, names)
    if header == "vd_hip.h":          # its where and pattern are the parser's defaults
        assert hip.parse_header("int vd_a(int n);") == {"vd_a": (_i, [_i])}
        with pytest.raises(ValueError, match=r"^include/vd_hip\.h: "):
            hip.parse_header("int vdk_a(int n);")


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


# header -> (the structs hip.py mirrors, the array bounds it restates, sizes pinned by hand), each under the header's own name
LAYOUTS = {"vd_hip.h": (["VdConvParams", "VdMatchSeg", "VdMatchBatch", "VdPackSeg", "VdPackBatch"], ["VD_PACK_MAX", "VD_MATCH_MAX_SEG"], {}),
           "vd_keyframes.h": (["VdkTable"], ["VDK_MAX_FRAMES"], {"VdkTable": 8 + 4 * 4 * 64}),
           "vd_frepo.h": (["VdfAdamSeg", "VdfAdamBatch"], ["VDF_ADAM_MAX"], {"VdfAdamSeg": 56, "VdfAdamBatch": 32 + 16 * 56})}


@pytest.mark.parametrize("header", list(LAYOUTS))
def test_mirrors_have_the_layout_the_compiler_gives_the_header(header, tmp_path):
    """A host program compiled from ``header`` alone prints sizeof of the structs the binding mirrors and offsetof / size of every
    field the mirrors name; the ctypes layout must be the same, and so must the array bounds."""
    from video_distillation_amd import hip
    structs, bounds, sizes = LAYOUTS[header]
    structs = [getattr(hip, s) for s in structs]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "%s"' % header, 'int main() {']
    lines += ['    std::printf("%s %%d\\n", %s);' % (b, b) for b in bounds]
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
    want = {b: "%d" % getattr(hip, b) for b in bounds}
    for s in structs:
        want[s.__name__] = "%d" % ctypes.sizeof(s)
        for f, offset, size in _mirror_fields(s):
            want["%s.%s" % (s.__name__, f)] = "%d %d" % (offset, size)
    assert got == want
    assert {name: ctypes.sizeof(getattr(hip, name)) for name in sizes} == sizes


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


HASHED = [("HEADERS", k, name) for k, name in enumerate(ABI)] + [("CSRC_HEADERS", k, name) for k, name in enumerate(["frame_norm.h", "split16.h"])] \
    + [("SOURCES", k, name) for k, name in enumerate(SOURCES)]


@pytest.mark.parametrize("table,k,name", HASHED, ids=["%s-%s" % (table, name) for table, _, name in HASHED])
def test_touching_a_file_moves_the_hashes_it_is_under(table, k, name, tmp_path, monkeypatch):
    """Row ``k`` of ``hip.HEADERS`` / ``CSRC_HEADERS`` / ``SOURCES`` is replaced by a touched copy.  A header moves
    ``sources_hash()`` and the key of every object; a source moves ``sources_hash()`` and the key of its own object only;
    undoing restores every value."""
    from video_distillation_amd import hip
    want, keys = hip.sources_hash(), [hip._object_key(src) for src in hip.SOURCES]
    assert len(set(keys)) == len(keys) == len(SOURCES)
    rows = list(getattr(hip, table))
    path = os.path.join(hip.INCLUDE, rows[k][0]) if table == "HEADERS" else rows[k]
    assert os.path.basename(path) == name
    copy = tmp_path / name
    copy.write_text(open(path).read() + "\n/* touched */\n")
    rows[k] = (str(copy), rows[k][1]) if table == "HEADERS" else str(copy)
    monkeypatch.setattr(hip, table, tuple(rows) if table == "HEADERS" else rows)
    assert hip.sources_hash() != want
    moved = [hip._object_key(src) != key for src, key in zip(hip.SOURCES, keys)]
    assert moved == ([j == k for j in range(len(keys))] if table == "SOURCES" else [True] * len(keys))
    monkeypatch.undo()
    assert hip.sources_hash() == want and [hip._object_key(src) for src in hip.SOURCES] == keys


def test_a_build_stamps_the_library_and_every_object_with_those_hashes():
    from video_distillation_amd import hip
    hip.build()
    assert hip.library_stamp() == hip.sources_hash()
    for src in hip.SOURCES:
        side = os.path.join(os.path.dirname(src), "build", os.path.basename(src) + ".o.srchash")
        if os.path.exists(side):          # (a library that was copied in has no object directory beside it)
            assert open(side).read().strip() == hip._object_key(src), src


def test_constants_mirrored_by_hand_equal_the_header_s_defines():
    """hip.py reads no file on import, so it restates a few of the header's ``#define``s; each is compared here."""
    import inspect
    from video_distillation_amd import hip
    defines = {}
    for path in hip.header_paths():
        text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
        found = re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VD[A-Z]?_\w+)[ \t]+(-?\d+)[ \t]*$", text, flags=re.M)
        assert not set(dict(found)) & set(defines), path
        defines.update((name, int(value)) for name, value in found)
    for name, value in (("VDK_MAX_FRAMES", 64), ("VDN_MAX_SYN", 1024), ("VDN_LDS_SYN", 128), ("VDF_ADAM_MAX", 16)):
        assert defines[name] == getattr(hip, name) == value, name
    from video_distillation_amd import keyframes
    assert keyframes.MAX_FRAMES == hip.VDK_MAX_FRAMES
    assert hip.PREC == {name[len("VD_PREC_"):].lower(): v for name, v in defines.items() if name.startswith("VD_PREC_")}
    assert len(hip.PREC) == 5 and sorted(hip.PREC.values()) == [0, 1, 2, 3, 4]
    assert hip.F16X3_WSHIFT == defines["VD_F16X3_WSHIFT"]
    assert (hip.PERSIST_GENS_MASK, hip.PERSIST_PLAIN_K, hip.PERSIST_NO_ALT) == (0xFFFF, 1 << 19, 1 << 20) == tuple(
        defines["VD_PERSIST_" + name] for name in ("GENS_MASK", "PLAIN_K", "NO_ALT"))
    assert hip.VD_PACK_MAX == defines["VD_PACK_MAX"] and hip.VD_MATCH_MAX_SEG == defines["VD_MATCH_MAX_SEG"]
    assert hip.CORESET_METHOD == {"herding": defines["VD_CORESET_HERDING"], "k-center": defines["VD_CORESET_KCENTER"]}
    assert defines["VD_ABI_VERSION"] == 5
    assert "vd_abi_version() != %d:" % defines["VD_ABI_VERSION"] in inspect.getsource(hip.lib)
