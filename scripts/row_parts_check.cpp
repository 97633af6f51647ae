// row_parts_check.cpp — prints part_rows (cutrace_amd/csrc/row_parts.h) over a range of frames for tests/test_row_parts_cpu.py:
// one line "h block_rows n_parts part row_begin row_end first_block n_rows" per case.  Host only: g++, no HIP.
#include <stdio.h>

#include <initializer_list>

#include "row_parts.h"

int main() {
  for (uint64_t h = 0; h <= 40; h++)
    for (uint64_t B = 1; B <= 9; B++)
      for (uint32_t n = 1; n <= 5; n++)
        for (uint32_t p = 0; p < n; p++)
          for (uint64_t begin : {(uint64_t)0, B, 2 * B})
            for (uint64_t end : {h, h - 3}) {
              if (end > h || (end != h && end == 0)) continue;  // h - 3 only where it is positive
              const PartRows r = part_rows(begin, end, B, p, n);
              printf("%llu %llu %u %u %llu %llu %llu %llu\n", (unsigned long long)h, (unsigned long long)B, n, p, (unsigned long long)begin,
                     (unsigned long long)end, (unsigned long long)r.first_block, (unsigned long long)r.n_rows);
            }
  return 0;
}
