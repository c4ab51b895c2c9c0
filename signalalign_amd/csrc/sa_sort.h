// The device-pointer form of sa_sort_u64 (sa_sort.hip), for stages that sort what already lies in HBM (sa_scores.hip).
#ifndef SA_SORT_H
#define SA_SORT_H

#include <stddef.h>
#include <stdint.h>

// bytes of working storage (digit counts, per-tile histograms, the scan's block sums) that a sort of n keys needs beside `tmp`
size_t sa_sort_work_bytes(size_t n);
// d_out[0 .. n) = d_in[0 .. n) ascending, on stream 0 of the current device.  d_in is not written; d_tmp holds n keys and d_work
// sa_sort_work_bytes(n) bytes, both 256-byte aligned; d_out, d_tmp and d_in are three different arrays.  n <= 2^31 - 1.  The call
// waits once for the device (the digit counts come back to choose the passes); the last pass may still be running when it returns.
// passes_out (may be NULL): the scatter passes that ran.
int sa_sort_u64_device(const uint64_t *d_in, size_t n, uint64_t *d_out, uint64_t *d_tmp, char *d_work, int *passes_out);

#endif
