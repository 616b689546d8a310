"""GPU: the pack refresh (csrc/vsde_pack.hip: pack_refresh_kernel) against the integer round-to-nearest-even bf16 cast of
tests/optimizer_reference.py: EXACT equality (a NaN must stay a NaN, its payload is free), in the pack and in its transposed copy.

Every case drives ``_hip.pack_refresh`` with a tile table built here, in the row layout of ``PackedWeight.refresh_all``
(src, dst, dst_t | 0, src_pitch, dst_pitch, pitch_t, rows | cols << 32, 0).  All tiles of a case live in three arenas -- fp32
sources, the packs, the transposed copies -- each tile's region on a 16-byte boundary with sentinel elements around it; the two
bf16 arenas are filled with the bit pattern 0x7FC1 and, after the launch, must hold the cast where a tile says so and the sentinel
everywhere else: the columns beyond ``cols``, the rows beyond ``rows`` (every pack region has 16 rows), the padded columns of
a 682 -> 768 pack, the neighbours of a transposed row run.  The sources must be unchanged.

Dispatch coverage (case -> path):

  test_tiles              rows 1 .. 16 x cols {1, 7, 255, 256, 257, 682, 1024}   threads without a column, one column each, a second trip
                          no dst_t; src_pitch = cols (whole parameter) and > cols (a row slice of a wider one)
                          dst_t at packed row 0, pitch_t 32        rows == 16: two 16-byte stores per column; rows < 16: scalar stores
                          dst_t at packed row 1, 4                 rows == 16 on the scalar transposed route (run not on 16 bytes)
                          dst_t at packed row 8, pitch_t 32 / 28   on 16 bytes again / only in every other column
                          dst_t at packed row 0, pitch_t 20        both routes inside one tile
                          cols 682 into a pack of pitch 768        the zero-padded SwiGLU pack: padding untouched
  test_bias_form          rows 1, all pitches = n
  test_values             every pattern class of optimizer_reference.pack_patterns in every one of the three store routes
  test_empty_table        0 tiles: no launch
  test_many_tiles         3000 tiles of 8 x 8
"""
import numpy as np
import pytest
import torch

import optimizer_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 16
SENT = np.uint16(R.PACK_SENTINEL)
COLS = (1, 7, 255, 256, 257, 682, 1024)


def tile(rows, cols, src_pitch=None, dst_pitch=None, t=None):
    """``t``: None or (pitch_t, first packed row of the run in the transposed copy)."""
    return {"rows": rows, "cols": cols, "src_pitch": src_pitch or cols, "dst_pitch": dst_pitch or cols, "t": t}


def run_tiles(tiles):
    """Lays the tiles out, runs ONE launch over them and compares all three arenas with the integer reference."""
    from viforsdes_amd import _hip
    vals = R.pack_values()
    up8 = lambda n: (n + 7) // 8 * 8
    cur = {"src": GUARD, "dst": GUARD, "t": GUARD}
    for i, tl in enumerate(tiles):
        assert 1 <= tl["rows"] <= 16 and tl["src_pitch"] >= tl["cols"] and tl["dst_pitch"] >= tl["cols"]
        tl["src0"], cur["src"] = cur["src"], up8(cur["src"] + tl["rows"] * tl["src_pitch"] + GUARD)
        tl["dst0"], cur["dst"] = cur["dst"], up8(cur["dst"] + 16 * tl["dst_pitch"] + GUARD)
        if tl["t"] is not None:
            pitch_t, row0 = tl["t"]
            assert row0 + 16 <= pitch_t                                # a 16-row run (the two 16-byte stores) stays inside its row
            tl["t0"], cur["t"] = cur["t"], up8(cur["t"] + tl["cols"] * pitch_t + GUARD)
    src = np.zeros(cur["src"], np.uint32)
    src[:] = 0x7FC54321                                               # NaN between the sources: a stray read shows
    want = {"dst": np.full(cur["dst"], SENT), "t": np.full(cur["t"], SENT)}
    nan = {k: np.zeros(a.size, bool) for k, a in want.items()}
    for i, tl in enumerate(tiles):
        rows, cols, sp, dp = tl["rows"], tl["cols"], tl["src_pitch"], tl["dst_pitch"]
        block = np.resize(np.roll(vals, -37 * i), rows * sp).reshape(rows, sp)
        src[tl["src0"]:tl["src0"] + rows * sp] = block.ravel()
        cast = R.bf16_rne_bits(block[:, :cols])
        is_nan = R.bf16_is_nan(cast)
        at = tl["dst0"] + np.arange(rows)[:, None] * dp + np.arange(cols)[None, :]
        want["dst"][at], nan["dst"][at] = cast, is_nan
        if tl["t"] is not None:
            pitch_t, row0 = tl["t"]
            at = tl["t0"] + row0 + np.arange(cols)[None, :] * pitch_t + np.arange(rows)[:, None]
            want["t"][at], nan["t"][at] = cast, is_nan
    d_src = torch.from_numpy(src.view(np.int32)).to(DEV)
    d_dst = torch.from_numpy(np.full(cur["dst"], SENT).view(np.int16)).to(DEV)
    d_t = torch.from_numpy(np.full(cur["t"], SENT).view(np.int16)).to(DEV)
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0 and d_t.data_ptr() % 16 == 0
    rows = [(d_src.data_ptr() + 4 * tl["src0"], d_dst.data_ptr() + 2 * tl["dst0"],
             0 if tl["t"] is None else d_t.data_ptr() + 2 * (tl["t0"] + tl["t"][1]),
             tl["src_pitch"], tl["dst_pitch"], 0 if tl["t"] is None else tl["t"][0], tl["rows"] | (tl["cols"] << 32), 0) for tl in tiles]
    table = torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 8).to(DEV)
    _hip.pack_refresh(table)
    torch.cuda.synchronize()
    assert np.array_equal(d_src.cpu().numpy().view(np.uint32), src)
    for k, dev in (("dst", d_dst), ("t", d_t)):
        got = dev.cpu().numpy().view(np.uint16)
        wrong = np.flatnonzero((got != want[k]) & ~nan[k])
        assert wrong.size == 0, (k, wrong[:8], [hex(x) for x in got[wrong[:8]]], [hex(x) for x in want[k][wrong[:8]]])
        assert R.bf16_is_nan(got[nan[k]]).all() and (got[nan[k]] != SENT).all(), k       # a NaN was written, and it is a NaN
    return want, nan


@pytest.mark.parametrize("rows", range(1, 17))
def test_tiles(rows):
    tiles = []
    for cols in COLS:
        padded = 768 if cols == 682 else cols + 3
        tiles += [tile(rows, cols), tile(rows, cols, src_pitch=cols + 5, dst_pitch=padded),
                  tile(rows, cols, dst_pitch=padded, t=(32, 0)), tile(rows, cols, src_pitch=cols + 5, t=(32, 1)),
                  tile(rows, cols, t=(32, 4)), tile(rows, cols, t=(32, 8)), tile(rows, cols, dst_pitch=padded, t=(28, 8)),
                  tile(rows, cols, t=(20, 0))]
    run_tiles(tiles)


def test_bias_form():
    run_tiles([tile(1, n) for n in (1, 64, 682, 768, 1365, R.pack_values().size)])


def test_values():
    """One tile per store route, wide enough to hold every pattern in every row (no two rows of a tile alike)."""
    n = R.pack_values().size
    wide = lambda rows, t: tile(rows, n, src_pitch=n + 1, t=t)          # the values repeat after n: every row starts one pattern later
    want, nan = run_tiles([wide(16, (16, 0)), wide(16, (24, 1)), wide(7, (8 + 16, 8)), wide(16, None)])
    assert nan["dst"].sum() == (16 + 16 + 7 + 16) * R.pack_patterns()["nan"].size
    for name, u in R.pack_patterns().items():                            # the classes reach the kernel as named
        assert np.isin(R.bf16_rne_bits(u)[~R.bf16_is_nan(R.bf16_rne_bits(u))], want["dst"]).all(), name


def test_empty_table():
    from viforsdes_amd import _hip
    _hip.pack_refresh(torch.zeros(0, 8, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()


def test_many_tiles():
    run_tiles([tile(8, 8, src_pitch=8 + i % 3, dst_pitch=8 + i % 2, t=(24, 8 * (i % 2)) if i % 4 else None) for i in range(3000)])
