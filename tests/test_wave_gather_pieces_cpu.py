"""The direct-to-LDS gather of the pipelined wave kernels in WHOLE-ROW pieces (csrc/mgp_fused_wave_kernel.h:
wave_gather_lane / wave_gather_on / wave_gather_whole_rows), restated in Python and checked without a GPU, as
tests/test_jit_cpu.py does for the pair scheme.

The image in LDS is row r at 16-byte slot r * spr (spr slots a row, the last one padding).  One gather instruction
(a piece) writes lane l's 16 bytes at the piece's base + 16 l.  Whole-row pieces start at row RPP * p, RPP = 64 // spr;
lanes RPP * spr .. 63, and lanes of the last piece whose row does not exist, are switched off.  Behind the tile lie the
row pointers the NEXT gather reads: a lane that writes there sends that gather to a stray address."""

import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "muygpys_amd", "csrc", "mgp_fused_wave_kernel.h")

# BASELINE.md's configs 2 to 5: (element size, nn_count, responses, features); config 5 has more than 64 slots -- it is
# no wave kernel's shape and drops out below
BASELINE_SHAPES = [(4, 30, 1, 40), (4, 30, 1, 40), (8, 50, 1, 8), (4, 64, 16, 40)]


def _modm(np_, k, gram):
    """wave_dims(): does the static pair scheme run modulo the k + 1 feature rows?"""
    need = (k + 1) // 2
    ba, bp = 4, (need + 3) // 4
    for c in (3, 5):
        q = (need + c - 1) // c
        if c * q < ba * bp:
            ba, bp = c, q
    return ba * bp + (2 if gram else 1) <= np_ // 2


def geometry(es, k, R, d, bwd=False):
    """(spr, rows the gather fills, rows of the tile, image-order pieces) of a static pipelined instantiation."""
    slots = k + 1 + R
    np_ = 16 if slots <= 16 else (32 if slots <= 32 else 64)
    assert slots <= 64
    E = 16 // es
    ch = 2 * E
    dlt = es == 8 and np_ == 64
    dcap = 128 if (bwd and not dlt and es == 4) else 64
    dst = min((d + ch - 1) // ch * ch, dcap)
    spr = (dst + E) // E
    nh = 64 // np_
    if nh > 1:
        return spr, 64, 64, spr
    pieces = ((k + 1) * spr + 63) // 64
    covered = (pieces * 64 + spr - 1) // spr
    live = slots if _modm(np_, k, gram=(es == 4)) else np_
    tile_rows = max(covered, live)
    return spr, min(pieces * 64 // spr, tile_rows), tile_rows, pieces


def lane_rule(lane, spr, last):
    rr = lane // spr
    return rr, min(lane - rr * spr, last), lane < (64 // spr) * spr


def lane_on(lane, p, spr, rows):
    rr, _, active = lane_rule(lane, spr, spr - 1)
    left = rows - (64 // spr) * p
    return active if left >= 64 // spr else (active and rr < left)


def row_pieces(rows, spr):
    return -(-rows // (64 // spr))


def whole_rows(rows, spr, image_pieces, num, den):
    return spr <= 64 and den * row_pieces(rows, spr) <= num * image_pieces


def check_cover(rows, spr, tile_rows):
    """Every slot of every gathered row once, nothing at or behind the end of the tile, no piece across a row."""
    rpp = 64 // spr
    hits = [0] * (rows * spr)
    for p in range(row_pieces(rows, spr)):
        first_row = None
        for lane in range(64):
            if not lane_on(lane, p, spr, rows):
                continue
            rr, c, _ = lane_rule(lane, spr, spr - 1)
            slot = p * rpp * spr + lane  # where the transfer puts the lane's 16 bytes
            assert slot < rows * spr <= tile_rows * spr, (rows, spr, p, lane)
            assert slot == (p * rpp + rr) * spr + c, (rows, spr, p, lane)  # slot c of row RPP p + rr: the row it fetched
            assert p * rpp <= slot // spr < (p + 1) * rpp  # whole rows of this piece only
            first_row = slot // spr if first_row is None else first_row
            hits[slot] += 1
        assert first_row == p * rpp
    assert hits == [1] * (rows * spr), (rows, spr)


def _static_shapes():
    from muygpys_amd import build

    shapes = {(es, k, R, d, False) for es, k, R, d in BASELINE_SHAPES if k + 1 + R <= 64}
    shapes |= {(4, k, 1, d, False) for k in build.PREWARM_K for d in build.PREWARM_D}
    shapes |= {(8, k, 1, d, False) for k in build.PREWARM_K for d in build.PREWARM_D if d <= 32}
    shapes |= {(es, k, 1, d, True) for es, k, d in build.PREWARM_BWD}
    return sorted(shapes)


def _rule_constants():
    text = open(HEADER).read()
    m = re.search(r"WAVE_GATHER_ROWS_NUM = (\d+), WAVE_GATHER_ROWS_DEN = (\d+);", text)
    assert m, "the selection rule's constants are named in the header"
    # ... and the rule is the one restated in whole_rows()
    assert re.search(r"WAVE_GATHER_ROWS_DEN \* wave_gather_row_pieces\(wave_gather_rows\(w, NP, KFIX, xs\), spr\) <= "
                     r"WAVE_GATHER_ROWS_NUM \* wave_gather_pieces\(w, KFIX, xs\)", text)
    return int(m.group(1)), int(m.group(2))


def test_whole_row_pieces_cover_every_static_shape_once_and_stay_inside_the_tile():
    num, den = _rule_constants()
    assert (num, den) == (5, 4)
    chosen = {}
    for es, k, R, d, bwd in _static_shapes():
        spr, rows, tile_rows, image_pieces = geometry(es, k, R, d, bwd)
        assert k + 1 <= rows <= tile_rows <= 64
        check_cover(rows, spr, tile_rows)  # (the rule must hold whether or not the instantiation selects it)
        chosen[(es, k, R, d, bwd)] = whole_rows(rows, spr, image_pieces, num, den)
    # where the line falls: the headline shape takes 13 pieces for 11, the 27-slot rows of the
    # d = 100 backward 32 for 27; three-slot rows (fp32, d = 8: 4 for 3) and 17-slot rows (d = 64: 22 for 17) keep the
    # image order
    assert chosen[(4, 30, 1, 40, False)] and geometry(4, 30, 1, 40)[:2] == (11, 64)
    assert row_pieces(64, 11) == 13 and row_pieces(64, 27) == 32
    assert not chosen[(4, 10, 1, 8, False)] and not chosen[(4, 30, 1, 64, False)]
    assert chosen[(4, 20, 1, 16, False)] and chosen[(8, 40, 1, 8, False)] and chosen[(4, 30, 1, 32, False)]
    assert chosen[(4, 30, 1, 100, True)]


@pytest.mark.parametrize("es", [4, 8])
def test_whole_row_pieces_cover_the_run_time_shape_geometries(es):
    """64 rows (NH * NP = 64), 2 .. 33 slots a row: the run-time-shape kernels keep the image order (64 * spr slots in
    spr pieces, nothing to switch off), but the rule itself must hold for every row length they can have."""
    for spr in range(2, 34):
        check_cover(64, spr, 64)
        # image order, restated: piece n covers slots 64 n .. 64 n + 63
        assert sorted(64 * n + lane for n in range(spr) for lane in range(64)) == list(range(64 * spr))


def test_last_piece_of_the_headline_shape_stops_at_the_row_pointers():
    """fp32, k = 30, d = 40: the tile ends at byte 11 264, where the 64 row pointers start.  Piece 12 holds rows 60 .. 63:
    lanes 0 .. 43 write, lanes 44 .. 54 (a fifth row) and 55 .. 63 must not."""
    spr, rows, tile_rows, _ = geometry(4, 30, 1, 40)
    assert (spr, rows, tile_rows) == (11, 64, 64)
    on = [lane for lane in range(64) if lane_on(lane, 12, spr, rows)]
    assert on == list(range(44))
    assert max(12 * 5 * spr * 16 + 16 * lane + 16 for lane in on) == 11264
    for p in range(12):
        assert [lane for lane in range(64) if lane_on(lane, p, spr, rows)] == list(range(55))


def _msgpack_uint_after(blob: bytes, key: str):
    k = bytes([0xA0 + len(key)]) + key.encode()
    i = blob.find(k)
    if i < 0:
        return None
    b = blob[i + len(k)]
    if b < 0x80:
        return b
    width = {0xCC: 1, 0xCD: 2, 0xCE: 4}.get(b)
    return int.from_bytes(blob[i + len(k) + 1:i + len(k) + 1 + width], "big") if width else None


def test_headline_kernels_keep_168_registers_three_waves_and_nothing_spills():
    import json

    from muygpys_amd import build

    build.build()
    res = json.load(open(os.path.join(build.LIBDIR, "kernel_resources.json")))
    headline = [k for k in res if re.search(r"fused_wave_kernelIfLi32ELi30ELi1ELi40ELb1ELb0ELb[01]ELb1ELb0ELb0EEE", k)]
    assert len(headline) == 2, sorted(res)
    for name in headline:
        r = res[name]
        assert r["VGPRs"] <= 168 and r["VGPRs Spill"] == 0 and r["ScratchSize [bytes/lane]"] == 0, (name, r)
        assert r["Occupancy [waves/SIMD]"] >= 3, (name, r)
    # the prewarmed forward shapes: no spilled register, no scratch (the code objects' own metadata)
    assert build.prewarm() > 0
    jit = os.path.join(build.LIBDIR, "jit")
    seen = 0
    for name in sorted(os.listdir(jit)):
        if not name.endswith(".hsaco") or "_b1_" in name:
            continue
        blob = open(os.path.join(jit, name), "rb").read()
        assert _msgpack_uint_after(blob, ".vgpr_spill_count") == 0, name
        assert _msgpack_uint_after(blob, ".private_segment_fixed_size") == 0, name
        seen += 1
    assert seen >= 60
