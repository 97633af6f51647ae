"""Host logic (CPU, no GPU): the row-partition rule the library's host code shares (cutrace_amd/csrc/row_parts.h: make_rows of
ctr_render.cpp, the part sizes of ctr_multi.hip) against its Python statement, cutrace_amd.tiling.part_rows, restricted to the row
range — every h in 0..40, block_rows in 1..9, n_parts in 1..5, every part, row_begin in {0, block_rows, 2 block_rows} and
row_end in {h, h - 3 where positive} (scripts/row_parts_check.cpp prints the cases)."""
from cutrace_amd.tiling import part_rows
from tests.checkers import I_CSRC, check_output, check_program


def test_shared_row_partition_equals_tiling_part_rows(tmp_path_factory):
    exe = check_program(tmp_path_factory, "row_parts_check", ("-O2", "-Wall", I_CSRC))
    lines = check_output(exe, timeout=60).splitlines()
    seen = set()
    for line in lines:
        h, B, n, p, begin, end, first_block, n_rows = (int(x) for x in line.split())
        mine = [y for y in part_rows(h, p, n, B) if begin <= y < end]
        assert n_rows == len(mine), line
        if mine:
            assert first_block == mine[0] // B, line
        seen.add((h, B, n, p, begin, end))
    want = {(h, B, n, p, begin, end) for h in range(41) for B in range(1, 10) for n in range(1, 6) for p in range(n)
            for begin in (0, B, 2 * B) for end in {h, h - 3} if end == h or end > 0}
    assert seen == want and len(lines) == len(want)
