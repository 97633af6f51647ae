// row_parts.h — the one row-partition rule of the host: which rows of a frame a part owns (needs no HIP).
//
// Rows are dealt in blocks of `block_rows`: block b = rows [b * block_rows, (b + 1) * block_rows) belongs to part
// b % n_parts.  cutrace_amd/tiling.py part_rows states the same rule in Python (tests/test_row_parts_cpu.py compares them).
#ifndef CUTRACE_AMD_ROW_PARTS_H
#define CUTRACE_AMD_ROW_PARTS_H

#include <stdint.h>

struct PartRows { uint64_t first_block, n_rows; };  // the part's first block at or after row_begin; how many rows it owns

// The rows of [row_begin, row_end) that part `part` of `n_parts` owns; row_begin is a multiple of block_rows (> 0).
inline PartRows part_rows(uint64_t row_begin, uint64_t row_end, uint64_t block_rows, uint32_t part, uint32_t n_parts) {
  const uint64_t b0 = row_begin / block_rows;
  PartRows r{b0 + ((part + n_parts - (b0 % n_parts)) % n_parts), 0};
  for (uint64_t b = r.first_block; b * block_rows < row_end; b += n_parts) {
    const uint64_t lo = b * block_rows, hi = lo + block_rows < row_end ? lo + block_rows : row_end;
    r.n_rows += hi - lo;
  }
  return r;
}

#endif
