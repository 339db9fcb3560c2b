// mt_markers.hip -- marker ids (include/mtgpu.h "marker ids"): MergeTree.posFromRelativePos
// (mergeTree.ts:1943-1966) for a batch of (document, view, key, value id) queries, one wave per query
// over the document's compact state in HBM.
//
// The reference looks the id up in a map and walks up from the marker (getPosition,
// mergeTree.ts:1586-1603), adding nodeLength of every earlier sibling on the way: the view lengths of
// the leaves before it.  Here the wave passes over the leaves once, 64 at a time, carrying the view's
// prefix; each lane keeps the best candidate among its leaves (mt_marker.h: the rule the apply engine
// resolves relative records by) together with that leaf's prefix, and the wave's choice is made once,
// after the last chunk.  No LDS, no atomics; per leaf it reads the fields mt_view_len reads, the
// flags, and -- for markers with properties only -- the words holding the key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgpu.h"
#include "mt_checksum.h"
#include "mt_launch.h"
#include "mt_marker.h"
#include "mt_state.h"
#include "mt_view.h"
#include "mt_wave.h"

// A query of a document >= n_docs or of a key past the wide form's: ordinal MT_POS_BAD_QUERY, nothing read.
__global__ __launch_bounds__(64) void mt_marker_positions_kernel(mt_gstate g, const mt_marker_query* __restrict__ q,
                                                                 uint32_t nq, uint32_t n_docs,
                                                                 mt_marker_result* __restrict__ out) {
    const uint32_t w = blockIdx.x;
    if (w >= nq) return;
    const int lane = lane_id();
    const mt_marker_query qq = q[w];
    if (qq.doc >= n_docs || qq.key >= MT_MAX_KEYS_WIDE) {  // (device-resident queries are not checked on the host)
        if (lane == 0) out[w] = mt_marker_result{MT_POS_BAD_QUERY, 0, 0u, 0u};
        return;
    }
    const mt_doc_scalars sc = g.sc[qq.doc];
    const int n = sc.nseg;
    const size_t so = (size_t)qq.doc * g.segcap;
    const mt_view view = mt_view_of(sc, qq.ref_seq, qq.client);
    mt_marker_best best;
    int best_prefix = 0, best_vl = 0;
    int carry = 0;  // the view's length before the chunk
    for (int base = 0; qq.value != 0 && base < n; base += 64) {
        const int i = base + lane;
        const int vl = i < n ? mt_view_len(g, view, so + i) : 0;
        const int incl = wave_incl_scan(vl);
        if (i < n) {
            const uint8_t f = g.flags[so + i];
            const bool cand = (f & MT_SF_MARKER) && (f & MT_SF_PDEF) && mt_gprop(g, view.form, so + i, qq.key) == qq.value;
            best.fold(cand, g.seq[so + i], i);
            if (best.ord == i) {
                best_prefix = carry + incl - vl;
                best_vl = vl;
            }
        }
        carry += wave_last(incl);
    }
    const int k = mt_marker_pick(best);
    if (k < 0) {
        if (lane == 0) out[w] = mt_marker_result{-1, 0, 0u, 0u};
        return;
    }
    if (best.ord == k) {  // the one lane that holds leaf k
        const uint32_t fl = (best_vl == 0 ? MT_MKF_HIDDEN : 0u) | ((g.flags[so + k] & MT_SF_REMOVED) ? MT_MKF_TOMBSTONE : 0u);
        out[w] = mt_marker_result{k, best_prefix, fl, g.len[so + k]};
    }
}

extern "C" hipError_t mt_launch_marker_positions(const mt_gstate* g, const mt_marker_query* q, uint32_t n, uint32_t n_docs,
                                                 mt_marker_result* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_marker_positions_kernel, dim3(n), dim3(64), 0, st, *g, q, n, n_docs, out);
    return hipGetLastError();
}
