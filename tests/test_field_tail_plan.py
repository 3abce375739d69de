"""tn_render_tail_segments / tn_render_tail_plan: how many sample segments the last partial round of a whole-march field call is
recorded in (no compute call: runs without a GPU)."""
import ctypes

from thermo_nerf_amd import _hip


def test_plan_table():
    lib = _hip.load()
    table = {(10000, 2048, 192): 9,   # 1 808 x 9 units = 7.95 rounds of one ninth
             (8192, 2048, 192): 1,    # no remainder
             (1250, 2048, 192): 1,    # no whole round: stays with the split form
             (10000, 2048, 12): 1}    # no two segments of 12 samples
    for (tiles, slots, S), want in table.items():
        assert lib.tn_render_tail_segments(tiles, slots, S, 0) == want, (tiles, slots, S)
        assert lib.tn_render_tail_segments(tiles, slots, S, 1) == 1
    # forced: k, or fewer where the segments would be shorter than 12 samples; never an empty segment
    assert [lib.tn_render_tail_segments(37, 16, 48, k) for k in (2, 3, 7, 16)] == [2, 3, 4, 4]
    assert [lib.tn_render_tail_segments(37, 16, S, 16) for S in (1, 2, 13, 23, 24, 192, 1024)] == [1, 1, 1, 1, 2, 16, 16]
    assert lib.tn_render_tail_segments(10000, 2048, 192, 13) == 13 and lib.tn_render_tail_segments(10000, 2048, 100, 7) == 7
    assert lib.tn_render_tail_segments(10000, 2048, 100, 8) == 8  # 8 segments of 13: 7 x 13 = 91 < 100
    assert lib.tn_render_tail_segments(10000, 2048, 50, 4) == 4 and lib.tn_render_tail_segments(10000, 2048, 49, 3) == 3
    # 9 segments of 11 would be shorter than 12: 8, whose 13-sample segments number ceil(100 / 13) = 8
    assert lib.tn_render_tail_segments(10000, 2048, 100, 9) == 8


def test_plan_of_a_call_and_its_workspace():
    lib = _hip.load()
    rc = _hip.tn_render_config()
    rc.num_proposal_samples[0], rc.num_proposal_samples[1], rc.num_nerf_samples = 256, 96, 192
    fld = _hip.tn_thermal_field()
    blob = (ctypes.c_float * 4)()
    fld.prepared = ctypes.addressof(blob)
    frame = 800 * 800
    rc.tail_balance = 1
    base = lib.tn_render_workspace_bytes(rc, frame)
    rc.tail_balance = 0
    assert lib.tn_render_tail_plan(fld, rc, frame) == lib.tn_render_tail_plan(None, rc, frame) == 9
    assert lib.tn_render_tail_records_bytes(rc, frame) == 1808 * 245760
    assert 0 <= lib.tn_render_workspace_bytes(rc, frame) - 1808 * 245760 - base < 256
    for field, value in (("tail_balance", 1), ("training", 1), ("early_stop_transmittance", 1e-3), ("kernel_family", 2)):
        saved = getattr(rc, field)
        setattr(rc, field, value)
        assert lib.tn_render_tail_plan(fld, rc, frame) == 1, field
        assert lib.tn_render_tail_records_bytes(rc, frame) == 0, field
        setattr(rc, field, saved)
    fld.prepared_f16x3 = ctypes.addressof(blob)  # the split-precision kernels march whole tiles
    assert lib.tn_render_tail_plan(fld, rc, frame) == 1
    fld.prepared_f16x3 = None
    # a call the sample_split form takes (tn_render_sample_split > 1) is not planned; forced to whole tiles it is
    assert lib.tn_render_sample_split(fld, rc, 5000 * 64) > 1 and lib.tn_render_tail_plan(fld, rc, 5000 * 64) == 1
    rc.sample_split = 1
    assert lib.tn_render_tail_plan(fld, rc, 5000 * 64) == lib.tn_render_tail_segments(5000, 2048, 192, 0) > 1
    rc.sample_split = 0
    rc.tail_slots, rc.kernel_family, rc.sample_split, rc.num_nerf_samples = 16, 1, 1, 48
    assert lib.tn_render_tail_plan(fld, rc, 37 * 64) == 3 and lib.tn_render_tail_records_bytes(rc, 37 * 64) == 5 * 48 * 1280
    assert lib.tn_render_tail_plan(None, None, frame) == 1 and lib.tn_render_tail_plan(fld, rc, 0) == 1


def test_workspace_layout_values():
    """tn_render_workspace_bytes / tn_render_tail_records_bytes of the library before the launchers shared one layout type: the
    literals were recorded from that build, never from the code under test."""
    lib = _hip.load()
    rays = (1, 63, 64, 65, 4096, 65536, 640000)
    table = {(256, 96, 48): (104960, 104960, 104960, 207872, 6588416, 105383936, 1029122048),
             (256, 96, 192): (141824, 141824, 141824, 281600, 8947712, 143132672, 1842096128),
             (64, 32, 48): (39424, 39424, 39424, 76800, 2394112, 38275072, 373762048)}
    records = {(256, 96, 192, 640000): 444334080}  # 1 808 tiles of the frame's fifth round; every other entry plans none
    for (P0, P1, S), want in table.items():
        rc = _hip.tn_render_config()
        rc.num_proposal_samples[0], rc.num_proposal_samples[1], rc.num_nerf_samples = P0, P1, S
        for R, total in zip(rays, want):
            assert lib.tn_render_workspace_bytes(rc, R) == total, (P0, P1, S, R)
            assert lib.tn_render_tail_records_bytes(rc, R) == records.get((P0, P1, S, R), 0), (P0, P1, S, R)
    # tail_slots = 8: 19 tiles are two full rounds + three tiles; (workspace, records, planned segments)
    small = {(256, 96, 48): (2141696, 184320, 2), (256, 96, 192): (3395072, 737280, 8), (64, 32, 48): (896512, 184320, 2)}
    for (P0, P1, S), (total, rec, k) in small.items():
        rc = _hip.tn_render_config()
        rc.num_proposal_samples[0], rc.num_proposal_samples[1], rc.num_nerf_samples = P0, P1, S
        rc.tail_slots, rc.kernel_family, rc.sample_split = 8, 1, 1
        assert lib.tn_render_workspace_bytes(rc, 19 * 64) == total, (P0, P1, S)
        assert lib.tn_render_tail_records_bytes(rc, 19 * 64) == rec, (P0, P1, S)
        assert lib.tn_render_tail_plan(None, rc, 19 * 64) == k, (P0, P1, S)
    assert lib.tn_render_workspace_bytes(None, 64) == 0 and lib.tn_render_workspace_bytes(rc, -1) == 0
