// mt_text.hip -- text reads (include/mtgpu.h "text reads"): MergeTreeTextHelper.getText /
// getTextAndMarkers (textSegment.ts:124-276) for a batch of (document, range, view) queries, one wave
// per query over the document's compact state in HBM.
//
// The reference walks mapRange -> nodeMap (mergeTree.ts:2903-2965) with gatherText as the leaf action
// (textSegment.ts:188-275).  Over the leaves in order, with p a leaf's exclusive prefix in the view and
// len its view length, nodeMap visits the leaf when end - p > 0 && len > 0 && start - p < len (a block
// that holds such a leaf passes the same test, so the blocks add nothing); a visited text segment gives
// text.substring(max(start - p, 0), end - p) -- units [min(a, b), max(a, b)) with a, b the two
// arguments clamped to [0, len], substring's argument swap included -- and a visited marker gives the
// placeholder cachedLength (1) times.
//
// Segments here are a few units long, so the copy is laid out by OUTPUT unit, not by segment: per chunk
// of 64 leaves one DPP scan gives each lane its leaf's view prefix and another its clipped unit
// count's output prefix; the chunk's output units are then dealt to the lanes in order (lane j takes
// units j, j + 64, ...), each lane finds its unit's source leaf by a six-step search over the 64
// output prefixes (ds_bpermute: the prefixes stay in registers, every lane reads another lane's
// dword, which the LDS crossbar serves without bank conflicts and without a barrier) and the stores
// of a step are 64 consecutive units whatever the segment lengths.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgpu.h"
#include "mt_checksum.h"
#include "mt_launch.h"
#include "mt_state.h"
#include "mt_view.h"
#include "mt_wave.h"

// row_ptr == nullptr: the count pass (counts[w] only).  Else the write pass: query w's units go to
// units[row_ptr[w] ..), at most row_ptr[w + 1] - row_ptr[w] of them, its marker rows to
// markers[m_row_ptr[w] ..) likewise (m_row_ptr == nullptr: none are written), and counts[w] is the
// whole count either way.  A query of a document >= n_docs: MT_TEXT_BAD_QUERY units, nothing read.
__global__ __launch_bounds__(64) void mt_text_ranges_kernel(mt_gstate g, const mt_text_query* __restrict__ q, uint32_t nq,
                                                            uint32_t n_docs, const uint32_t* __restrict__ row_ptr,
                                                            uint16_t* __restrict__ units,
                                                            const uint32_t* __restrict__ m_row_ptr,
                                                            mt_text_marker* __restrict__ markers,
                                                            mt_text_count* __restrict__ counts) {
    const uint32_t w = blockIdx.x;
    if (w >= nq) return;
    const int lane = lane_id();
    const mt_text_query qq = q[w];
    const uint32_t d = qq.doc;
    if (d >= n_docs) {  // (device-resident queries are not checked on the host)
        if (lane == 0) counts[w] = mt_text_count{MT_TEXT_BAD_QUERY, 0u};
        return;
    }
    const mt_doc_scalars sc = g.sc[d];
    const int n = sc.nseg;
    const size_t so = (size_t)d * g.segcap;
    const mt_view view = mt_view_of(sc, qq.ref_seq, qq.client);
    const int64_t start = qq.start, end = qq.end;  // (64-bit: start - p of any two int32 values)
    const int64_t stop = start > end ? start : end;
    const uint32_t ph = qq.placeholder;
    const bool want_markers = (qq.flags & MT_TEXT_MARKERS) != 0;
    const uint32_t lo = row_ptr ? row_ptr[w] : 0u;
    const uint32_t room = row_ptr ? row_ptr[w + 1] - lo : 0u;
    const uint32_t mlo = (row_ptr && m_row_ptr) ? m_row_ptr[w] : 0u;
    const uint32_t mroom = (row_ptr && m_row_ptr) ? m_row_ptr[w + 1] - mlo : 0u;
    const uint8_t* __restrict__ arena = g.text + ((size_t)d * 2 + sc.text_half) * g.textcap;
    int64_t vcarry = 0;            // the view's length before the chunk
    uint32_t total = 0, mtotal = 0;  // units / marker rows before the chunk
    for (int base = 0; base < n && vcarry < stop; base += 64) {
        const int i = base + lane;
        const int vl = i < n ? mt_view_len(g, view, so + i) : 0;
        const int vincl = wave_incl_scan(vl);
        const int vsum = wave_last(vincl);
        if (vcarry + vsum <= start) {  // wholly before start: p + len <= start for each of its leaves
            vcarry += vsum;
            continue;
        }
        const int64_t p = vcarry + vincl - vl;
        const bool visited = vl > 0 && end - p > 0 && start - p < vl;
        const bool marker = visited && (g.flags[so + i] & MT_SF_MARKER) != 0;
        int cnt = 0;
        uint32_t src = 0;  // the arena unit of the leaf's first output unit
        if (marker) {
            cnt = ph ? 1 : 0;
        } else if (visited) {
            auto clamped = [vl](int64_t x) -> int64_t { return x < 0 ? 0 : x > vl ? vl : x; };
            const int64_t a = clamped(start - p), b = clamped(end - p);
            cnt = (int)(a < b ? b - a : a - b);
            src = g.toff[so + i] + (uint32_t)(a < b ? a : b);
        }
        const int oincl = wave_incl_scan(cnt);  // (a wave's leaves hold far less than 2^31 units)
        const int oexcl = oincl - cnt;
        const int T = wave_last(oincl);
        const uint64_t mm = wave_ballot(marker && want_markers);
        if (mm) {
            if (marker && want_markers) {
                const uint32_t k = mtotal + (uint32_t)__popcll(mm & ((1ull << lane) - 1ull));
                if (k < mroom) markers[mlo + k] = mt_text_marker{i, total + (uint32_t)oexcl};
            }
            mtotal += (uint32_t)__popcll(mm);
        }
        if (room > total) {  // the write pass, with room left in the row
            const int delta = (int)src - oexcl;  // output unit k of the chunk comes from arena unit delta + k
            for (int kb = 0; kb < T; kb += 64) {  // (uniform: every lane takes part in the search)
                const int k = kb + lane;
                int j = 0;  // the first leaf of the chunk whose inclusive output prefix exceeds k
                for (int step = 32; step; step >>= 1)
                    if (__shfl(oincl, j + step - 1, 64) <= k) j += step;
                const int dj = __shfl(delta, j, 64);
                const int mj = __shfl((int)marker, j, 64);
                if (k < T && total + (uint32_t)k < room) {
                    uint32_t u = ph;
                    if (!mj) {
                        const uint32_t at = (uint32_t)(dj + k);
                        u = view.wdoc ? (uint32_t)reinterpret_cast<const uint16_t*>(arena)[at] : (uint32_t)arena[at];
                    }
                    units[(size_t)lo + total + (uint32_t)k] = (uint16_t)u;
                }
            }
        }
        total += (uint32_t)T;
        vcarry += vsum;
    }
    if (lane == 0) counts[w] = mt_text_count{total, mtotal};
}

extern "C" hipError_t mt_launch_text_ranges(const mt_gstate* g, const mt_text_query* q, uint32_t n, uint32_t n_docs,
                                            const uint32_t* row_ptr, uint16_t* units, const uint32_t* m_row_ptr,
                                            mt_text_marker* markers, mt_text_count* counts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_text_ranges_kernel, dim3(n), dim3(64), 0, st, *g, q, n, n_docs, row_ptr, units, m_row_ptr, markers,
                       counts);
    return hipGetLastError();
}
