"""numpy interpreter of the tile program that csrc/conv_mfma.hip executes on the GPU.

It consumes exactly the tables the device consumes (ConvPlan.flat_tables(), boxes, widx) and
follows the same dataflow (patch gather with zero fill -> per-row/tap A operand -> K-step
products -> pooled / row epilogue), in fp64, so that the planner can be checked on the CPU.
"""
import numpy as np

from video_distillation_amd import plan as P


def pack_weights(plan, w_flat):
    """[CC,S,NT,64,8] operand values (what vd_pack_weights writes, before 16-bit rounding)."""
    idx = plan.widx
    out = np.where(idx >= 0, w_flat[np.maximum(idx, 0)], 0.0)
    return out


def run_plan(plan, src, w_flat, bias, nclips, out):
    """src: float array [nclips, CC, ...] whose trailing dims flatten to the 16-bit ELEMENTS of one
    channel chunk (2 per dword); out: flat float64 array (pre-zeroed).
    Returns argmax array (same indexing as out) for pooled epilogues."""
    descs, tables = plan.flat_tables()
    wp = pack_weights(plan, w_flat)                       # [CC,S,NT,64,8]
    lane = np.arange(64)
    col, half = lane & 31, lane >> 5
    arg = {}
    gather = plan.gather_table()
    src_flat = src.reshape(src.shape[0], src.shape[1], -1)
    ngroups = -(-nclips // plan.ncl)
    for grp in range(ngroups):
        clip0 = grp * plan.ncl
        for bi, box in enumerate(plan.boxes):
            ty, f0, h0, w0, out_rel, _ = [int(v) for v in box]
            pf, ph, pw, pitch_h, pitch_f, pitch_c, mt, a_ofs, o_ofs, t_ofs = [int(v) for v in descs[ty][:10]]
            a_off = tables[a_ofs:a_ofs + mt * 32] // 16
            tap_off = tables[t_ofs:t_ofs + 2 * plan.S] // 16
            pos = plan.epi == P.EPI_POS_FEAT        # position tiles: skip masks behind the taps, B operands per box, pool across tiles
            skip = tables[t_ofs + 2 * plan.S:t_ofs + 2 * plan.S + plan.S // 4] if pos else None
            nout = mt * 4 if plan.epi != P.EPI_ROWS else mt * 32
            out_tab = tables[o_ofs:o_ofs + nout]
            acc = np.zeros((mt * 32, plan.NT * 32))
            for cc in range(plan.CC):
                patch = np.zeros((plan.ncl * pitch_c + 64, 8))
                gt = gather[bi]
                for idx in range(plan.ncl * pitch_c):
                    e = int(gt[idx])
                    if e < 0:
                        continue
                    b = clip0 + (e >> 24)
                    if b >= nclips:
                        continue
                    o2 = 2 * (e & 0xFFFFFF)                   # dword offset -> element offset
                    assert 0 <= o2 and o2 + 8 <= src_flat.shape[2], \
                        "%s box %d slot %d gathers elements [%d, %d) of a %d-element chunk" % (plan.name, bi, idx, o2, o2 + 8, src_flat.shape[2])
                    patch[idx] = src_flat[b, cc, o2:o2 + 8]
                # A[row, s, half, j]
                for s in range(plan.S):
                    for hh in range(2):
                        lanes = np.where(half == hh)[0]
                        if pos:
                            for i in range(mt):
                                if (int(skip[s // 4]) >> i) & 1:
                                    continue
                                sl = a_off[i * 32:(i + 1) * 32] + tap_off[2 * s + hh]
                                assert sl.min() >= 0 and sl.max() < plan.ncl * pitch_c, "position tile reads outside its patch"
                                for nt in range(plan.NT):
                                    acc[i * 32:(i + 1) * 32, nt * 32:(nt + 1) * 32] += patch[sl] @ wp[bi * plan.CC + cc, s, nt, lanes, :].T
                            continue
                        a = patch[a_off + tap_off[2 * s + hh]]            # [rows, 8]
                        for nt in range(plan.NT):
                            bmat = wp[cc, s, nt, lanes, :]                 # [32 cols, 8]
                            acc[:, nt * 32:(nt + 1) * 32] += a @ bmat.T
            n = np.arange(plan.NT * 32)
            nvalid = n < plan.n_out
            if bias is not None:
                acc = acc + np.where(nvalid, np.pad(bias, (0, max(0, plan.NT * 32 - bias.size)))[:plan.NT * 32], 0.0)[None, :]
            if plan.relu:
                acc = np.maximum(acc, 0.0)
            if pos:
                for e in range(16):
                    o = int(out_tab[e])
                    if o < 0 or clip0 + o // plan.out_clip_stride >= nclips:
                        continue
                    rows = [i * 32 + 2 * e + d for i in range(mt) for d in range(2)]
                    out[clip0 * plan.out_clip_stride + out_rel + o + n * plan.n_stride] = acc[rows].max(axis=0)
            elif plan.epi == P.EPI_ROWS:
                for r in range(mt * 32):
                    o = int(out_tab[r])
                    if o < 0:
                        continue
                    base = clip0 * plan.out_clip_stride + out_rel + o
                    ci = o // plan.out_clip_stride
                    if clip0 + ci >= nclips:
                        continue
                    coff = plan.col_off[n[nvalid]] if plan.col_off is not None else n[nvalid] * plan.n_stride
                    out[base + coff] = acc[r, nvalid]
            else:
                for t in range(mt):
                    for q in range(4):
                        o = int(out_tab[t * 4 + q])
                        if o < 0:
                            continue
                        ci = o // plan.out_clip_stride
                        if clip0 + ci >= nclips:
                            continue
                        rows = [t * 32 + P._row_of(q, j) for j in range(8)]
                        vals = acc[rows]                                   # [8, N]
                        sets = [(0, slice(0, 8))] if plan.pool_t == 2 else [(0, slice(0, 4)), (1, slice(4, 8))]
                        for dt, sl in sets:
                            v = vals[sl]
                            mx, am = v.max(axis=0), v.argmax(axis=0)
                            base = clip0 * plan.out_clip_stride + out_rel + o + dt * (-plan.out_t_stride if (plan.pair_flip >> q) & 1 else plan.out_t_stride)
                            if plan.epi == P.EPI_POOL_FEAT:
                                out[base + n * plan.n_stride] = mx
                                for k in n:
                                    arg[base + k * plan.n_stride] = am[k]
                            else:   # CL slots: chunk = n//8, element n%8
                                idxs = (base + (n // 8) * plan.out_chunk_stride) * 8 + (n % 8)
                                out[idxs] = mx
                                for k, ii in zip(n, idxs):
                                    arg[ii] = am[k]
    return arg


def clip_minor(x, nclips):
    """What vd_clip_minor_cl / _pix produce (before 16-bit rounding): [cin][clip/8][t*h*w][8 clips], absent clips zero."""
    cin = x.shape[1]
    ccb = -(-nclips // 8)
    out = np.zeros((cin, ccb * 8, int(np.prod(x.shape[2:]))))
    out[:, :nclips] = np.asarray(x, dtype=np.float64)[:nclips].reshape(nclips, cin, -1).transpose(1, 0, 2)
    return out.reshape(cin, ccb, 8, -1).transpose(0, 1, 3, 2).copy()


def run_wgrad_plan(plan, x, dy, nclips):
    """The weight-gradient tile program (plan.plan_wgrad) in fp64, from the tables the device reads: flat_tables(), gather_table(),
    ``boxes`` (word 5 = accumulation copy) and the packed-dy layout of plan.wgrad_pack_index.
    x (nclips, cin, t, h, w), dy (nclips, cout, T, OH, OW) -> dW (cout, cin, 3, 7, 7).

    A 'clip' of the program is an input channel, its channel chunks are the chunks of 8 clips of the clip-minor source; per box
    the patch is gathered with zero fill, K step s / lane half hh multiplies A = patch[a_off + tap_off[2 s + hh]] (rows = taps, 8
    clips) by the box's packed dy (32 output channels x 8 clips per N tile), and the live rows of the row table are added into
    copy box[5] of the [cin][tap][cout] target; the copies are folded at the end."""
    descs, tables = plan.flat_tables()
    gather = plan.gather_table()
    src = clip_minor(x, nclips)                             # [cin, CCb, npos, 8]
    cin = src.shape[0]
    src_flat = src.reshape(cin, plan.CC, -1)               # 16-bit ELEMENTS of one (channel, clip chunk)
    assert src.shape[1] == plan.CC and plan.ncl == 1 and plan.epi == P.EPI_ROWS and plan.atomic and plan.n_stride == 1
    dyf = np.asarray(dy, dtype=np.float64)[:nclips].transpose(0, 2, 3, 4, 1).reshape(-1)          # [clip][t][oh][ow][n]
    idx = P.wgrad_pack_index(plan)                          # [nbox, CCb, S, NT, 64, 8]
    assert idx.max() < dyf.size
    assert plan.w_box_stride == plan.CC * plan.S * plan.NT * 64 * 8
    replicas = int(plan.meta["replicas"])
    ncol = plan.NT * 32
    assert ncol == plan.n_out
    rep = np.zeros((replicas, cin * plan.out_clip_stride))
    k8 = np.arange(8)
    for bi, box in enumerate(plan.boxes):
        ty, out_rel, copy = int(box[0]), int(box[4]), int(box[5])
        assert 0 <= copy < replicas, "box %d accumulates into copy %d of %d" % (bi, copy, replicas)
        pitch_c, mt, a_ofs, o_ofs, t_ofs = [int(v) for v in descs[ty][5:10]]
        a_off, rem_a = np.divmod(tables[a_ofs:a_ofs + mt * 32].astype(np.int64), 16)
        tap_off, rem_t = np.divmod(tables[t_ofs:t_ofs + 2 * plan.S].astype(np.int64), 16)
        assert not rem_a.any() and not rem_t.any(), "LDS offsets are whole 16-byte slots"
        out_tab = tables[o_ofs:o_ofs + mt * 32].astype(np.int64)
        live = np.where(out_tab >= 0)[0]
        assert live.size == 147 and (out_tab[live] == np.arange(147) * plan.n_out).all(), "147 live rows at tap * cout"
        gt = gather[bi][:pitch_c].astype(np.int64)
        fill = np.where(gt >= 0)[0]
        assert ((gt[fill] >> 24) == 0).all(), "one 'clip' (input channel) per box"
        o2 = 2 * (gt[fill] & 0xFFFFFF)                      # dword offset -> element offset
        assert fill.size == 0 or (o2.min() >= 0 and o2.max() + 8 <= src_flat.shape[2]), \
            "%s box %d gathers elements up to %d of a %d-element chunk" % (plan.name, bi, o2.max() + 8, src_flat.shape[2])
        sl = a_off[live][None, :] + tap_off[:, None]        # [2S, 147] patch slots of (step position, tap row)
        assert sl.min() >= 0 and sl.max() < pitch_c, "%s box %d reads slot %d of a %d-slot patch" % (plan.name, bi, sl.max(), pitch_c)
        for cb in range(plan.CC):
            patch = np.zeros((cin, pitch_c, 8))
            patch[:, fill] = src_flat[:, cb][:, o2[:, None] + k8[None, :]]
            bsel = idx[bi, cb]                              # [S, NT, 64, 8]
            bop = np.where(bsel >= 0, dyf[np.maximum(bsel, 0)], 0.0)
            # K index = (step s, lane half hh, clip k); a lane's column is lane & 31
            bmat = bop.reshape(plan.S, plan.NT, 2, 32, 8).transpose(0, 2, 4, 1, 3).reshape(plan.S * 16, ncol)
            amat = patch[:, sl].transpose(0, 2, 1, 3).reshape(cin * 147, plan.S * 16)      # [(channel, tap row), K]
            acc = (amat @ bmat).reshape(cin, 147, ncol)
            for c in range(cin):
                base = c * plan.out_clip_stride + out_rel
                rep[copy, (base + out_tab[live])[:, None] + np.arange(ncol)[None, :]] += acc[c]
    dw = rep.sum(axis=0).reshape(cin, 147, plan.n_out)
    return dw.transpose(2, 0, 1).reshape(plan.n_out, cin, P.KT, P.KH, P.KW)


def pix_to_rows(x_btchw):
    """What vd_pix2rows produces: [B, 1, T*3, H, pitch] with 3 leading zero pixels per row."""
    B, T, C, H, W = x_btchw.shape
    pitch = P.pix_row_pitch(W)
    out = np.zeros((B, 1, T * C, H, pitch))
    out[..., 3:3 + W] = x_btchw.reshape(B, 1, T * C, H, W)
    return out
