"""The per-clip slot counts every engine call path sizes its workspace views from (engine.clip_slots, read once by
EmbedEngine.__init__) against the two things they must agree with: where the forward programs WRITE (the plans' clip stride,
which is also what the C handle's layout uses) and the pixel-row format vd_pix2rows fills."""
import pytest

from video_distillation_amd import engine, plan as P


@pytest.mark.parametrize("geom", [(4, 64, 64), (8, 64, 64), (8, 80, 96), (16, 112, 112)])
def test_clip_slot_counts_match_the_forward_plans(geom):
    geo = P.NetGeometry(*geom)
    fwd = P.plan_network(geo)["fwd"]
    per0, per1, per2 = engine.clip_slots(geo, fwd)
    frames, height, width = geom
    assert per0 == frames * 3 * height * (P.pix_row_pitch(width) // 8)
    assert (per1, per2) == (fwd[0].out_clip_stride, fwd[1].out_clip_stride)
    # the next level reads what the previous one wrote: its source clip stride is in 4-byte units, a slot has 16 bytes
    assert (fwd[1].clip_stride4, fwd[2].clip_stride4) == (4 * per1, 4 * per2)
