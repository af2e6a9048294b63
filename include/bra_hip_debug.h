/*
 * bra_hip_debug.h -- diagnostic entry points of libbra_hip.so that are not part of the drop-in
 * C-ABI of bra_hip.h (tests/test_abi.py pins that header's function list); used by the tests.
 */
#pragma once

#include "bra_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * The first BWT split of the last batch encode on the context: *path = 1 when rotations were placed
 * by their first two packed key bytes in one pass (every block had between 2 and 8192 distinct
 * 16-bit packed prefixes and at least 16384 bytes; BRA_L0_WIDE=0, read when the context is created,
 * turns this off), 0 for the 8-bit level 0; *max_bins = the largest prefix count of one block (0
 * when the call did not build the prefix maps; exact up to 8704, a lower bound above 8704 for a
 * block with more).  Returns 0, -1 on a null argument.
 */
int bra_gpu_debug_bwt_path(bra_gpu_ctx_t* ctx, unsigned* path, unsigned* max_bins);

/*
 * The last inverse BWT on the context (a batch decode; call it after that call has returned).
 * *path: 0 none yet, 1 the main path (splitter walk staged in slots and overflow chunks), 2 the
 * two-walk path chosen directly (a block of 2^24 bytes or more), 3 the main path followed by the
 * two-walk fallback because the overflow pool ran out.  *walk, for paths 1 and 3: 0 one transform
 * step per load, 1 two steps per load, 2 one step because a block of the batch did not suit pairs
 * (read from the device by this call); 0 for path 2.  *pool_used: 256-byte overflow chunks the walk
 * asked for (it keeps counting past the capacity); *pool_cap: chunks the pool held.  Both 0 for
 * path 2.  Returns 0, -1 on a null argument or a failed device read.
 */
int bra_gpu_debug_ibwt_path(bra_gpu_ctx_t* ctx, unsigned* path, unsigned* walk, unsigned* pool_used, unsigned* pool_cap);

#ifdef __cplusplus
}
#endif
