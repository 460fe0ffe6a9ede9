"""The strip schedule's launch geometry as the kernels' headers state it (csrc/sdp_hard.h, csrc/sdp_soft_local.h), read from
the headers themselves, and the shapes that put a launch on the routes no small shape reaches.  TESTS ONLY.

One wave per strip of STRIP rows, at most MAX_WAVES waves per workgroup, one boundary row of M + STRIP floats per wave in LDS
plus 2 * MAX_WAVES progress words; the host lowers the wave count until that fits LDS_BUDGET (csrc/sdp_api.hip: hard_waves,
soft_local_waves)."""
import math
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "deepblast_amd" / "csrc"
# (N, M) -> (strips, waves): the full 64 KB launch; strip 7 is wave 0's second strip, one row high; the column limit with 66
# chunks to a strip, two waves wrap the ring of seven
WIDE = {(449, 1982): (8, 8), (449, 1983): (8, 7), (513, 2048): (9, 7)}


def constants(header):
    """the `constexpr int` constants of a header -> dict; the two formulas the rule below repeats must stand in it as they do here"""
    text = (CSRC / header).read_text()
    c = {}
    for name, expr in re.findall(r"constexpr int (\w+) = ([0-9 *]+);", text):      # a number, or a product of numbers
        c[name] = math.prod(int(x) for x in expr.split("*"))
    assert "row_pitch(int M) { return M + STRIP; }" in text, header
    assert "(int waves, int M) { return (size_t)waves * row_pitch(M) * 4 + 2 * MAX_WAVES * 4; }" in text, header
    return c


def lds_bytes(c, waves, M):
    return waves * (M + c["STRIP"]) * 4 + 2 * c["MAX_WAVES"] * 4


def strips(c, N):
    return (N + c["STRIP"] - 1) // c["STRIP"]


def chunks(c, m):
    return (m + c["STRIP"] - 1 + c["CHUNK"] - 1) // c["CHUNK"]


def waves(c, N, M):
    w = min(strips(c, N), c["MAX_WAVES"])
    while w > 1 and lds_bytes(c, w, M) > c["LDS_BUDGET"]:
        w -= 1
    return w


def check_wide_shapes(header):
    """the arithmetic that makes the wide shapes what they are: a change of pitch or budget fails here instead of silently moving
    the cases off their routes"""
    c = constants(header)
    assert (c["STRIP"], c["CHUNK"], c["MAX_WAVES"], c["LDS_BUDGET"]) == (64, 32, 8, 65536)
    assert 8 * (1982 + 64) * 4 + 64 == 65536 == lds_bytes(c, 8, 1982) == c["LDS_BUDGET"]       # the largest launch there is
    assert 8 * (1983 + 64) * 4 + 64 > 65536 and lds_bytes(c, 8, 1983) > c["LDS_BUDGET"] >= lds_bytes(c, 7, 2048)
    for (N, M), (S, W) in WIDE.items():
        assert (strips(c, N), waves(c, N, M)) == (S, W), (N, M)
    assert waves(c, 448, 1983) == 7 and waves(c, 449, 1982) == 8 and waves(c, 100000, 2048) == 7
    assert chunks(c, 2048) == 66 < c["KEY"] and (449 - 1) % 7 == 0 and 449 - 7 * 64 == 1      # strip 7: wave 0 again, one row
    return c
