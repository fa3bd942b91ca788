"""ONE forward level of csrc/conv_mfma.hip alone -- ``eng.fwd[li].run(...)`` on a freshly built source, never ``eng.forward`` --
against fp64, and bit for bit on integers.

The forward is otherwise seen only through three stacked levels and one rel-L2 over 256 to 2048 features
(tests/test_gpu_embed.py): a wrong tap at one border position of level 0, a mis-addressed row of the last (ragged) box or a
pooled window whose second frame lies ``out_t_stride`` the wrong way is diluted far below those limits.  Here every program
family runs on its own level's inputs (tests/forward_level_cases.py), in every format it runs in, through BOTH epilogues: the
staged one (``argmax = None``: whole 16-byte slots through LDS, the ``emit_lo`` low plane, ``vd_conv0_breg`` at level 0) and
the per-lane one (with arg-max buffers).  The output buffers hold one guard clip more than the batch and are prefilled with
sentinels (0x7FFF in 16-bit planes, NaN in fp32 features, 0x55 in arg-max bytes): afterwards the guard is untouched, no
sentinel remains in any owned element of any plane, and every arg-max byte has bits 3..6 clear (bit 2 too where pool_t = 1).

(A) EXACT ARITHMETIC.  Integer pixels, weights k/64, biases j/64: every partial sum of every order is exact in fp32, so the
    device must reproduce the fp64 value EXACTLY: every 16-bit plane is ``split16`` of it bit for bit (hi, lo of the hi+lo
    formats, the ``emit_lo = 1`` plane of a single-pass level 1; the only freedom is the sign of a zero), the fp32 features are
    its fp32 cast, the ``emit_lo = 1`` run's hi plane is the ``emit_lo = 0`` run's, live arg-max bytes are the FIRST maximum
    (ties included), the dead flag is ``value <= 0`` (exact zeros included).
(B) RANDOM DATA against the free fp64 value (the maximum over a window is 1-Lipschitz: no routing allowance), against the fp64 conv
    value at the recorded position, the decisions against the near-tie rule of tests/argmax_tools.py; the staged run equals the
    per-lane run as values.  The near-tie rule (tie_tol = 2e-5 x rms of the conv output) is stated against the free fp64 reference
    for the hi+lo formats; for the single-pass formats against the fp64 level on the operands AS THE FORMAT HOLDS THEM
    (forward_level_cases.format_reference): 11 resp. 8 operand bits alone route some 2e-4 resp. 2e-3 of the windows otherwise,
    with margins up to 7e-4 resp. 9e-3 x rms (asserted on the CPU: no program of such a format can meet 2e-5 against unrounded
    operands; measured on the device against them: f16 247 of 1.5e6 windows, worst margin 7.4e-4; bf16 1008 of 8.1e5, 6.0e-3 --
    printed per case).  Against the rounded operands only the fp32 accumulation is left: no window of any case is routed
    otherwise without being a near-tie, in any format.
(C) THE SELECT EPILOGUE of ``train.GradMatchEngine(...).sel[0..2]``, run directly with ``src_split_off4`` set as ``_up_sweep``
    sets it: P(conv(a, V) + conv(gbar, W)) * scale + vb with the arg-max bytes as an INPUT (dead windows among them), operands
    ``torch.cat([V, W], dim=1)``, one source at level 0.  Exact integers bit for bit (fp32 ``select = 2`` output of f16x3
    levels 0 and 1, fp32 features at level 2, split16 planes of bf16x3 ``select = 1``); random data at the bound of a single linear
    program.  64 x 64 x 8 and 65 x 63 x 4 (levels 1 / 2: 8 resp. 2 M tiles per wave), level 1 at 104 x 112 x 4 (7 M tiles, as at
    112 x 112 x 16) and level 2 at 112 x 112 x 16 (8 M tiles, two clips per box); one clip more than a box holds.

Program families (asserted per case in FAMILY: a planner change is a named failure, not a silently different test):
level 0 frame tiles (64 x 66 x 4, 65 x 63 x 4, 64 x 64 x 8; hi+lo: the plane-sequential instantiation; single pass: vd_conv0_breg
when staged, the generic kernel with arg-max) and four box types (70 x 58 x 4: the generic kernel in single pass too); level 1
NTW 2 / MTW 4 (64 x 66 x 4, 64 x 64 x 8), NTW 1 / MTW 2 in 3 boxes (70 x 58 x 4), NTW 1 / MTW 7 (hi+lo) and the balanced 7-tile
layout (single pass) at 104 x 112 x 4 -- a small clip size whose level 1 plans to them, 3 boxes instead of the 14 of
112 x 112 x 16; level 2 NTW 1 / MTW 2 with 8 clips per box (64 x 66 x 4), 4 (64 x 64 x 8: two pooled frames), 3 boxes (96 x 80 x 12),
NTW 2 / MTW 4 with 2 clips per box (112 x 112 x 16: no smaller size reaches it); the ``fwd2_hilo`` program of
``EmbedEngine(prec="f16", last_hilo=True)`` on a hi+lo source; the latency-oriented programs of ``batch_hint = 8`` at
112 x 112 x 16, levels 1 and 2.  Clips: 1 and 3 at level 0 (one clip per box: no group to make ragged), above it one more than a
box holds, and one alone where a box holds several.

Bounds of (B).  Starting point: what the project holds a single conv program to against fp64 -- rel-L2 f16x3 2e-5, bf16x3 1e-4,
f16 2e-3, bf16 2e-2, max-abs ratio 4 x that.  Rule (tests/test_gpu_input_gradient.py): a bound stays where the measured worst is
within ten times of it, otherwise it is four times the measured worst.  tests/test_forward_level_cpu.py recomputes what the
operand and output formats ALONE cost on these inputs and asserts that each bound leaves a factor of four over it.
MEASURED on an MI355X, worst over all cases (rel-L2 whole / border shell / max-abs ratio / at the recorded positions):
    f16x3   level 0  1.90e-07 / 1.65e-07 / 5.54e-07 / 1.90e-07    level 1  6.64e-07 / 6.60e-07 / 1.98e-06 / 6.64e-07
            level 2  7.89e-07 / 7.89e-07 / 2.12e-06 / 7.89e-07    -> 2e-5 was 25 x the worst: bound 4 x 7.89e-07 = 3.2e-6
    bf16x3  level 0  3.34e-06 / 3.27e-06 / 7.11e-06 / 3.34e-06    level 1  3.42e-06 / 3.42e-06 / 6.79e-06 / 3.42e-06
            level 2  2.55e-06 / 2.55e-06 / 4.37e-06 / 2.55e-06    -> 1e-4 was 29 x the worst: bound 4 x 3.42e-06 = 1.4e-5
    f16     level 0  2.56e-04 / 2.52e-04 / 4.96e-04 / 2.56e-04    level 1  2.61e-04 / 2.61e-04 / 4.27e-04 / 2.61e-04
            level 2  1.63e-04 / 1.63e-04 / 2.73e-04 / 1.64e-04    -> 2e-3 is 7.7 x the worst: stays
    bf16    level 0  2.04e-03 / 2.00e-03 / 3.51e-03 / 2.04e-03    level 1  2.06e-03 / 2.06e-03 / 3.55e-03 / 2.06e-03
            level 2  1.33e-03 / 1.33e-03 / 2.51e-03 / 1.33e-03    -> 2e-2 is 9.7 x the worst: stays
(the single-pass figures ARE their formats' floors -- the CPU companion finds 2.61e-04 and 2.08e-03 for the formats alone; the
fwd2_hilo program, alone and fed by an emit_lo = 1 level 1, and the latency-oriented programs lie inside the f16x3 / f16 rows.)
Select epilogue (rel-L2 whole / border shell / max-abs ratio):
    f16x3   level 0  1.77e-07 / 1.56e-07 / 4.15e-07    level 1  1.03e-06 / 1.03e-06 / 2.31e-06    level 2  1.09e-06 / 1.09e-06 / 3.11e-06
            -> 2e-5 was 18 x the worst: bound 4 x 1.09e-06 = 4.4e-6
    bf16x3  level 0  4.04e-06 / 3.86e-06 / 6.40e-06    level 1  4.45e-06 / 4.45e-06 / 7.43e-06    level 2  3.33e-06 / 3.33e-06 / 4.33e-06
            -> 1e-4 was 22 x the worst: bound 4 x 4.45e-06 = 1.8e-5
Every exact case of (A) and (C) passed bit for bit as first written: these tests found no defect in a kernel, the planner or the engine.
"""
import pytest
import torch

from tests import forward_level_cases as C

pytestmark = pytest.mark.gpu

G_A, G_B, G_C, SMALL, ODD, FULL, M7 = C.G_A, C.G_B, C.G_C, C.SMALL, C.ODD, C.FULL, C.M7

BOUND = C.BOUND                # relative L2 of one level against fp64 (module docstring; shared with tests/test_forward_level_cpu.py)

WORST = {}                    # (format, level) -> [rel-L2, shell, max-abs ratio, routed] seen so far
_ENGINES = {}

# (clip size, level, hi+lo?) -> (NTW, MTW, MW, clips per box, boxes, box types); None for hi+lo?: both
FAMILY = {
    (G_A, 0, None): (1, 4, 2, 1, 16, 1), (G_B, 0, None): (1, 4, 2, 1, 16, 1), (SMALL, 0, None): (1, 4, 2, 1, 32, 1),
    (G_C, 0, None): (1, 4, 2, 1, 18, 4),
    (G_A, 1, None): (2, 4, 2, 1, 1, 1), (SMALL, 1, None): (2, 4, 2, 1, 2, 1), (G_C, 1, None): (1, 2, 1, 1, 3, 1),
    (M7, 1, True): (1, 7, 1, 1, 3, 1), (M7, 1, False): (2, 3, 2, 1, 3, 1),
    (G_A, 2, None): (1, 2, 1, 8, 1, 1), (SMALL, 2, None): (1, 2, 1, 4, 1, 1), (ODD, 2, None): (1, 2, 1, 8, 3, 1),
    (FULL, 2, None): (2, 4, 2, 2, 1, 1),
}
LATENCY = {1: (1, 2, 1, 1, 49, 1), 2: (1, 2, 1, 1, 2, 1)}          # batch_hint = 8 at 112 x 112 x 16


def _engine(geom, fmt, batch_hint=None, last_hilo=False):
    from video_distillation_amd import engine, plan
    key = (geom, fmt, batch_hint, last_hilo)
    if key not in _ENGINES:
        _ENGINES[key] = engine.EmbedEngine(plan.NetGeometry(*geom), prec=fmt, device="cuda:0", batch_hint=batch_hint, last_hilo=last_hilo)
    return _ENGINES[key]


def _family(dp):
    pl = dp.plan
    return (pl.NTW, pl.MTW, pl.MW, pl.ncl, pl.nbox, len(pl.types))


def _assert_family(eng, dp, geom, li, fmt):
    x3 = C.planes_of(fmt) == 2
    want = FAMILY.get((geom, li, None)) or FAMILY[(geom, li, x3)]
    assert _family(dp) == want, "the planner moved %s level %d (%s) to %s, the test expects %s" % (geom, li, fmt, _family(dp), want)
    d = eng.dims[li]
    assert tuple(dp.plan.out_shape) == ((d[1], d[8], d[9], d[10]) if li == 2 else (d[1] // 8, d[8], d[9], d[10], 8))
    if li == 0:
        assert (dp.plan.NT, dp.plan.S) == (2, 32)
        frame_tiles = geom != G_C
        assert (dp.plan.meta.get("frame_tiles") == 1) == frame_tiles and (dp.plan.pair_flip != 0) == frame_tiles
        assert dp.breg_ok == (frame_tiles and not x3)          # vd_conv0_breg when staged; the generic kernel with four box types
        if x3:      # the plane-sequential instantiation: one channel chunk and clip per box, the staged hi+lo tiles fit one patch plane
            assert dp.plan.CC == 1 and 2 * dp.plan.MW * dp.plan.MTW * 4 * 2 * dp.plan.NT * 32 * 2 <= dp.params.lds_plane_bytes
    if geom == M7 and not x3:
        assert dp.plan.meta.get("balanced") == 1


def _source(eng, li, case, src_fmt):
    """The level's source, freshly built: fp32 clips through vd_pix2rows at level 0 (as EmbedEngine.forward does), channels-last
    16-bit slots above.  -> (tensor on the device, slots per plane)"""
    from video_distillation_amd import hip
    nb = case.nb
    if li == 0:
        g = eng.geo
        x = case.x.permute(0, 2, 1, 3, 4).contiguous().cuda()          # (nb, T, 3, H, W)
        rows = torch.empty((eng.planes, nb * eng.per0, 8), dtype=torch.int16, device="cuda")
        hip.run("vd_pix2rows", hip.ptr(x), hip.ptr(None), nb, g.frames, g.height, g.width, hip.ptr(rows[0]),
                hip.ptr(rows[1] if eng.planes == 2 else None), eng.prec, hip.stream_ptr(eng.device))
        torch.cuda.synchronize()
        return rows, nb * eng.per0
    slots = C.to_slots(case.x, src_fmt).cuda()
    return slots, int(slots.shape[1])


def _run(eng, dp, li, case, fmt, keep, emit_lo=0, src=None, weights=None):
    """One launch of the level's program into sentinel-filled buffers with a guard clip.  -> the buffers, on the host"""
    nb, dims = case.nb, eng.dims[li]
    src, n_src = src or _source(eng, li, case, fmt)
    planes_out = 2 if (emit_lo or C.planes_of(fmt) == 2) else 1
    out = C.output_buffers(dims, li, nb, planes_out, keep)
    dst = (out.feat if li == 2 else out.planes).cuda()
    am = out.am.cuda() if keep else None
    w, b = (case.w if weights is None else weights).contiguous().cuda(), case.b.cuda()
    dp.pack(w)
    dp.run(src, n_src, b, dst.data_ptr(), 0 if li == 2 else int(dst.shape[1]), am, nb, emit_lo=emit_lo)
    torch.cuda.synchronize()
    if li == 2:
        out.feat = dst.cpu()
    else:
        out.planes = dst.cpu()
    if keep:
        out.am = am.cpu()
    return out


def _clips(dp, nb):
    return dp.plan.ncl + 1 if nb == "ncl+1" else nb


def _cases():
    both, four = ("f16x3", "f16"), ("f16x3", "f16", "bf16x3", "bf16")
    out = []
    for geom, fmts in ((G_A, both), (G_B, four), (G_C, both), (SMALL, four)):
        out += [(geom, fmt, 0, nb) for fmt in fmts for nb in (1, 3)]
    for geom, fmts in ((G_A, both), (SMALL, four), (G_C, four), (M7, both)):
        out += [(geom, fmt, 1, "ncl+1") for fmt in fmts]
    for geom, fmts in ((G_A, both), (SMALL, four), (ODD, four), (FULL, both)):
        out += [(geom, fmt, 2, nb) for fmt in fmts for nb in ("ncl+1", 1)]
    return out


_IDS = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)          # noqa: E731


def _exact(eng, dp, li, case, fmt):
    """(A) for one program: staged and per-lane epilogue, and the low plane of a single-pass level 1."""
    staged = _run(eng, dp, li, case, fmt, keep=False)
    C.check_exact(staged, case, fmt)
    C.check_exact(_run(eng, dp, li, case, fmt, keep=True), case, fmt)
    if li == 1 and C.planes_of(fmt) == 1 and dp is eng.fwd[1]:
        pl = dp.plan
        tiles = pl.MW * pl.MTW + (1 if (pl.NTW == 2 and pl.MTW == 3) else 0)
        assert 2 * tiles * 4 * pl.NT * 32 * 2 <= dp.params.lds_plane_bytes, "the staged hi+lo tile no longer fits this program's patch plane"
        both = _run(eng, dp, li, case, fmt, keep=False, emit_lo=1)
        C.check_exact(both, case, fmt)                                  # hi and lo plane: split16 of the fp64 value
        assert torch.equal(both.planes[0], staged.planes[0]), "emit_lo = 1 changed the hi plane"


def _random(eng, dp, li, case, fmt, label, bound_fmt=None):
    """(B) for one program."""
    rec = WORST.setdefault((bound_fmt or fmt, li), [0.0, 0.0, 0.0, 0.0])
    bound = BOUND[bound_fmt or fmt]
    dref = C.format_reference(case, fmt) if C.planes_of(fmt) == 1 else None          # (single pass: the near-tie rule on the operands as held)
    lane = C.check_random(_run(eng, dp, li, case, fmt, keep=True), case, fmt, bound, label + ", per lane", rec, decisions_ref=dref)
    staged = C.check_random(_run(eng, dp, li, case, fmt, keep=False), case, fmt, bound, label + ", staged", rec)
    assert torch.equal(staged, lane), "the staged and the per-lane epilogue differ in %d values" % int((staged != lane).sum())


@pytest.mark.parametrize("geom,fmt,li,nb", _cases(), ids=_IDS)
def test_exact_inputs_give_the_fp64_level_bit_for_bit(geom, fmt, li, nb):
    eng = _engine(geom, fmt)
    dp = eng.fwd[li]
    _assert_family(eng, dp, geom, li, fmt)
    _exact(eng, dp, li, C.exact_case(geom, li, _clips(dp, nb)), fmt)


@pytest.mark.parametrize("geom,fmt,li,nb", _cases(), ids=_IDS)
def test_random_inputs_against_fp64(geom, fmt, li, nb):
    eng = _engine(geom, fmt)
    dp = eng.fwd[li]
    _assert_family(eng, dp, geom, li, fmt)
    nb = _clips(dp, nb)
    _random(eng, dp, li, C.random_case(geom, li, nb), fmt, "%s x %d clips" % (geom, nb))


@pytest.mark.parametrize("fmt", ["f16x3", "f16"])
@pytest.mark.parametrize("li", [1, 2])
def test_latency_oriented_programs(li, fmt):
    """batch_hint = 8 at 112 x 112 x 16 re-plans levels 1 and 2 for short workgroups (plan.latency_variant): (A) and (B)."""
    eng = _engine(FULL, fmt, batch_hint=8)
    dp = eng.fwd[li]
    assert _family(dp) == LATENCY[li] and _family(dp) != _family(_engine(FULL, fmt).fwd[li])
    _exact(eng, dp, li, C.exact_case(FULL, li, 2), fmt)
    _random(eng, dp, li, C.random_case(FULL, li, 2), fmt, "%s x 2 clips, batch_hint 8" % (FULL,))


def test_alternative_last_level_plan_on_a_hilo_source():
    """The ``fwd2_hilo`` program of EmbedEngine(prec="f16", last_hilo=True) at 112 x 112 x 16: fp16 hi+lo activations times fp16
    hi+lo weights -- (A), and (B) at the hi+lo bound of the level; then fed by an ``emit_lo = 1`` level 1: the two planes that
    producer wrote, read as the pair they are, against the fp64 level on their decoded sum."""
    eng = _engine(FULL, "f16", last_hilo=True)
    dp = eng.fwd2x
    assert dp.plan.name == "fwd2_hilo" and dp.prec == C.PREC["f16x3"] and (dp.plan.NTW, dp.plan.MTW) == (1, 4)
    nb = dp.plan.ncl + 1
    _exact(eng, dp, 2, C.exact_case(FULL, 2, nb), "f16x3")
    _random(eng, dp, 2, C.random_case(FULL, 2, nb), "f16x3", "%s x %d clips, fwd2_hilo" % (FULL, nb))
    # the producer: level 1 in single pass with the low plane of its outputs
    p1 = C.random_case(FULL, 1, nb)
    made = _run(eng, eng.fwd[1], 1, p1, "f16", keep=False, emit_lo=1)
    C.check_written(made, eng.dims[1], 1, nb)
    plain = _run(eng, eng.fwd[1], 1, p1, "f16", keep=False)
    assert torch.equal(made.planes[0], plain.planes[0]), "emit_lo = 1 changed the hi plane"
    d1 = eng.dims[1]
    per = (d1[1] // 8) * d1[8] * d1[9] * d1[10]
    pair = C.from_slots(made.planes, nb, d1[1], d1[8], d1[9], d1[10])
    mid = C.decode(pair, "f16")                              # what level 2 reads: hi + lo
    c2 = C.random_case(FULL, 2, nb)
    ref = C.reference(C.conv64(mid, c2.w), c2.b, eng.dims[2][11])
    src = made.planes[:, :nb * per].contiguous().cuda()
    out = _run(eng, dp, 2, c2, "f16x3", keep=False, src=(src, nb * per))
    C.check_random(out, c2, "f16x3", BOUND["f16x3"], "%s x %d clips, fwd2_hilo fed by emit_lo = 1" % (FULL, nb),
                   WORST.setdefault(("f16x3", 2), [0.0] * 4), ref=ref)


# ---- (C) the select epilogue ------------------------------------------------------------------------------------------------------
SELECT_WORST = {}             # (format, level) -> [rel-L2, shell, max-abs ratio] seen so far
_MATCHERS = {}
# (clip size, level) -> (NTW, MTW, MW, clips per box, boxes, box types) of train.GradMatchEngine.sel[level]; level 0 is the forward's plan
SELECT_FAMILY = {(SMALL, 1): (1, 8, 1, 1, 2, 1), (G_B, 1): (1, 8, 1, 1, 1, 1), (M7, 1): (1, 7, 1, 1, 3, 1),
                 (SMALL, 2): (1, 2, 1, 4, 1, 1), (G_B, 2): (1, 2, 1, 8, 1, 1), (FULL, 2): (1, 8, 1, 2, 1, 1)}


def _matcher(geom, fmt):
    from video_distillation_amd import plan, train
    if (geom, fmt) not in _MATCHERS:
        _MATCHERS[(geom, fmt)] = train.GradMatchEngine(plan.NetGeometry(*geom), 4, (1, 1, 1), "cuda:0", prec=fmt)
    return _MATCHERS[(geom, fmt)]


def _run_select(gm, li, case, fmt):
    """sel[li] run directly, with ``src_split_off4`` set as ``_up_sweep`` sets it: the two sources are the halves of one allocation.
    -> (output buffer on the host, mode)"""
    from video_distillation_amd import hip
    eng, dp, nb, dims = gm.eng, gm.sel[li], case.nb, gm.eng.dims[li]
    if li == 0:
        g = eng.geo
        x = case.a.permute(0, 2, 1, 3, 4).contiguous().cuda()
        src = torch.empty((eng.planes, nb * eng.per0, 8), dtype=torch.int16, device="cuda")
        hip.run("vd_pix2rows", hip.ptr(x), hip.ptr(None), nb, g.frames, g.height, g.width, hip.ptr(src[0]), hip.ptr(src[1]), eng.prec,
                hip.stream_ptr(eng.device))
        n_src, w = nb * eng.per0, case.V
    else:
        both = torch.stack([C.to_slots(case.a, fmt), C.to_slots(case.g, fmt)]).contiguous().cuda()          # [a | gbar][planes][nb * per][8]
        src, n_src = both[0], int(both.shape[2])
        off = both[1].data_ptr() - both[0].data_ptr()
        assert off > 0 and off % 4 == 0
        dp.params.src_split_off4 = off // 4
        w = torch.cat([case.V, case.W], dim=1)
    mode = "feat" if li == 2 else ("f32" if dp.params.select == 2 else "planes")
    assert dp.params.select == (2 if (fmt == "f16x3" and li < 2) else 1)
    buf = C.select_buffers(dims, li, nb, mode).cuda()
    n = dims[1] * dims[8] * dims[9] * dims[10]
    am = torch.full(((nb + 1) * n,), C.SENT_AM, dtype=torch.uint8)
    am[:nb * n] = case.am.reshape(-1) if li == 2 else C.bytes_to_slots(case.am)
    amd = am.cuda()
    scale = torch.tensor([C.SELECT_SCALE, 1.0 / C.SELECT_SCALE], dtype=torch.float32, device="cuda")
    dp.pack(w.contiguous().cuda())
    dp.run(src, n_src, case.vb.cuda(), buf.data_ptr(), int(buf.shape[1]) if mode == "planes" else 0, amd, nb, out_scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(amd.cpu(), am), "the select program wrote into its arg-max bytes"
    return buf.cpu(), mode


def _select_cases():
    out = [(geom, fmt, li) for geom in (SMALL, G_B) for fmt in ("f16x3", "bf16x3") for li in range(3)]
    return out + [(M7, "f16x3", 1), (M7, "bf16x3", 1), (FULL, "f16x3", 2)]


@pytest.mark.parametrize("geom,fmt,li", _select_cases(), ids=_IDS)
def test_select_epilogue_is_the_fp64_linear_operator(geom, fmt, li):
    """P(conv(a, V) + conv(gbar, W)) * scale + vb with the routing GIVEN: bit for bit on integers (fp32 ``select = 2`` output of
    f16x3 levels 0 and 1, fp32 features at level 2, split16 planes of bf16x3 ``select = 1``), and random data at the bound of a
    single linear program -- no allowance for a pooling decision, there is none."""
    gm = _matcher(geom, fmt)
    dp = gm.sel[li]
    if li == 0:
        assert dp.plan is gm.eng.fwd[0].plan
    else:
        assert _family(dp) == SELECT_FAMILY[(geom, li)], (_family(dp), SELECT_FAMILY[(geom, li)])
        assert dp.params.src_split_cc == gm.eng.dims[li][0] // 8
    nb = dp.plan.ncl + 1
    exact = C.select_case(geom, li, nb, "exact")
    buf, mode = _run_select(gm, li, exact, fmt)
    C.check_select(buf, exact, fmt, mode)
    rand = C.select_case(geom, li, nb, "random")
    buf, mode = _run_select(gm, li, rand, fmt)
    C.check_select(buf, rand, fmt, mode, C.SELECT_BOUND[fmt], "%s x %d clips" % (geom, nb), SELECT_WORST.setdefault((fmt, li), [0.0] * 3))
