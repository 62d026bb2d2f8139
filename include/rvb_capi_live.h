/* rvb_capi_live.h — what exact mode listed: a diagnostic for the live list of the fused impulse-response stage.  An extension of
 * rvb_capi.h (which it includes and whose types, codes and conventions it uses), exported by the same librvb_hip.so; rvb_capi.h itself
 * is unchanged by it.  No reference counterpart.  python: capi.Context.ir_exact_list_info.
 */
#ifndef RVB_CAPI_LIVE_H
#define RVB_CAPI_LIVE_H

#include "rvb_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

struct rvb_ctx;                   /* the context of rvb_capi.h */

/* The list of the last RVB_IR_EXACT binning or exact-mode prepare call on this context (RVB_ERR_STATE: there has been none;
 * RVB_HRTF_SPLIT_EARS=1 leaves none).  Exact mode sorts a list of the impulses that carry volume, not of all of them: the trace counts
 * its live diffuse impulses, the count comes down with the trace's small result block, and the list has room for that many and for every
 * image source.  The key pass counts the live impulses again per tile of RVB_LIVE_TILE records; the live ones are then written to the
 * list tile by tile and the rest of it is filled with entries that match no bin.
 *   *listed          entries of the list (per ear for the HRTF model): count + image sources, or every impulse where *count_valid == 0
 *   *live_on_device  impulses with volume that the key pass found (diffuse and images): never above *listed; waits for the stream
 *   *count_valid     0: the trace's count did not hold any more when the list was made (a source directivity, a re-shade or a relisten
 *                    had rewritten the records behind it), or RVB_SORT=own keeps the list of every impulse (then *live_on_device = *listed)
 * Any pointer may be NULL. */
#define RVB_LIVE_TILE 1024        /* records per tile of the live list; tests choose their edge shapes from it */
int rvb_ir_exact_list_info(rvb_ctx * ctx, uint64_t * listed, uint64_t * live_on_device, int * count_valid);

#ifdef __cplusplus
}
#endif

#endif
