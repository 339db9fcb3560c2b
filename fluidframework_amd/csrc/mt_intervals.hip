// mt_intervals.hip -- interval collections (include/mtgpu.h "interval collections"): the per-document
// table of (start reference, end reference, intervalType) beside the reference table of mt_refs.hip,
// add / remove by position, the overlap query and the positions of a document's intervals.
//
// The reference keeps SequenceIntervals in an augmented red-black tree of live reference objects
// (intervalCollection.ts:264-366, collections.ts:1027-1108) whose order and min/max go stale as the
// references move; the table here has no order at all.  A query evaluates the reference's own
// per-interval predicate, SequenceInterval.overlaps (intervalCollection.ts:149-156) over
// LocalReference.compare (localReference.ts:49-61), on every live entry at the references' current
// (ordinal, raw offset): lanes over the entries, 64 at a time.  Nothing here runs inside an apply; the
// references themselves are moved by the fold of mt_refs.hip, which every call runs first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgpu.h"
#include "mt_launch.h"
#include "mt_state.h"
#include "mt_wave.h"

namespace {

// A LocalReference as compare sees it: its segment's ordinal among the linked leaves (-1: undefined)
// and its raw offset (`offset`, not getOffset(): it counts on a tombstone and survives a detach)
struct End {
    int ord;
    uint32_t off;
};

// LocalReference.compare (localReference.ts:49-61): the same segment, or both undefined: by offset;
// an undefined segment sorts below every segment; else the order of the segments among the leaves
MT_DEV int cmp(const End a, const End b) {
    if (a.ord == b.ord) return (a.off > b.off) - (a.off < b.off);
    if (a.ord < 0) return -1;
    if (b.ord < 0) return 1;
    return a.ord < b.ord ? -1 : 1;
}

MT_DEV End end_of(const mt_ref* __restrict__ tab, uint32_t h, uint32_t refcap) {
    if (h >= refcap) return End{-1, 0u};
    const mt_ref r = tab[h];
    if (!(r.flags & MT_RF_LIVE)) return End{-1, 0u};  // (removed behind the collection's back)
    return End{r.ord >= 0 ? r.ord : -1, r.off};
}

// getContainingSegment(p0) and (p1) of document d's local view (client.ts:1004-1007) in one pass
// over its leaves in 64-leaf chunks that carries the view's prefix; whole wave, uniform arguments.
// A position below 0 or at / past the view's length has no segment: (-1, 0), as
// createPositionReference makes it (intervalCollection.ts:192-205).
MT_DEV void resolve2(const mt_gstate& g, uint32_t d, int p0, int p1, End& a, End& b) {
    a = End{-1, 0u};
    b = End{-1, 0u};
    const int lane = lane_id();
    const int n = g.sc[d].nseg;
    const size_t so = (size_t)d * g.segcap;
    bool need0 = p0 >= 0, need1 = p1 >= 0;
    int carry = 0;
    for (int base = 0; base < n && (need0 || need1); base += 64) {
        const int i = base + lane;
        const int ll = (i < n && !(g.flags[so + i] & MT_SF_REMOVED)) ? (int)g.len[so + i] : 0;
        const int incl = carry + wave_incl_scan(ll);
        if (need0) {
            const uint64_t m = wave_ballot(i < n && p0 < incl);
            if (m) {
                const int l = first_lane(m);
                a = End{base + l, (uint32_t)(p0 - __builtin_amdgcn_readlane(incl - ll, l))};
                need0 = false;
            }
        }
        if (need1) {
            const uint64_t m = wave_ballot(i < n && p1 < incl);
            if (m) {
                const int l = first_lane(m);
                b = End{base + l, (uint32_t)(p1 - __builtin_amdgcn_readlane(incl - ll, l))};
                need1 = false;
            }
        }
        carry = wave_last(incl);
    }
}

}  // namespace

// mt_intervals_overlapping, the hot path: one wave per query.  The query's transient interval is
// (getContainingSegment(start), getContainingSegment(end)) (findOverlappingIntervals,
// intervalCollection.ts:295-310); entry x matches when x.start.compare(q.end) < 0 &&
// x.end.compare(q.start) >= 0.  Matching handles are ballot-compacted in ascending order.
// row_ptr == nullptr: the count pass (counts[w] only).  Else the write pass: handles go to
// out[row_ptr[w] ..), at most row_ptr[w + 1] - row_ptr[w] of them; counts[w] is the whole count
// either way.  A query of a document >= n_docs, or of one without intervals, answers empty; only the
// intervals of the query's collection are seen.
__global__ __launch_bounds__(64) void mt_intervals_overlap_kernel(mt_gstate g, const mt_interval_query* __restrict__ q,
                                                                  uint32_t nq, uint32_t n_docs,
                                                                  const uint32_t* __restrict__ row_ptr,
                                                                  uint32_t* __restrict__ counts, uint32_t* __restrict__ out) {
    const uint32_t w = blockIdx.x;
    if (w >= nq) return;
    const int lane = lane_id();
    const mt_interval_query qq = q[w];
    const uint32_t d = qq.doc;
    uint32_t total = 0;
    if (d < n_docs && g.ivn[d] != 0) {
        End qs, qe;
        resolve2(g, d, qq.start, qq.end, qs, qe);
        const mt_interval* __restrict__ iv = g.ivs + (size_t)d * g.ivcap;
        const mt_ref* __restrict__ tab = g.refs + (size_t)d * 2 * g.refcap;
        const uint32_t lo = row_ptr ? row_ptr[w] : 0u;
        const uint32_t room = row_ptr ? row_ptr[w + 1] - lo : 0u;
        for (uint32_t base = 0; base < g.ivcap; base += 64) {
            const uint32_t h = base + lane;
            bool hit = false;
            if (h < g.ivcap) {
                const mt_interval x = iv[h];
                if (x.live && (x.type >> 16) == qq.collection) {
                    const End s = end_of(tab, x.start, g.refcap), e = end_of(tab, x.end, g.refcap);
                    hit = cmp(s, qe) < 0 && cmp(e, qs) >= 0;
                }
            }
            const uint64_t m = wave_ballot(hit);
            if (hit) {
                const uint32_t k = total + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (k < room) out[lo + k] = h;
            }
            total += (uint32_t)__popcll(m);
        }
    }
    if (lane == 0) counts[w] = total;
}

extern "C" hipError_t mt_launch_intervals_overlap(const mt_gstate* g, const mt_interval_query* q, uint32_t n,
                                                  uint32_t n_docs, const uint32_t* row_ptr, uint32_t* counts,
                                                  uint32_t* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_intervals_overlap_kernel, dim3(n), dim3(64), 0, st, *g, q, n, n_docs, row_ptr, counts, out);
    return hipGetLastError();
}

// mt_intervals_add, after mt_resolve_kernel answered getContainingSegment of both positions
// (at[2 * w], at[2 * w + 1]): one thread per interval claims an entry of its document's interval
// table, then its two references as mt_refs_claim_kernel does (pending until the next fold; one with
// no containing segment is born detached: ord -1, off 0, in no collection, so not pending).  A full
// table of either kind gives MT_REF_FULL and what was claimed is handed back: no half-made interval
// and no stray reference stay behind.
__global__ void mt_intervals_claim_kernel(mt_gstate g, const mt_interval_add* __restrict__ in,
                                          const mt_pos_result* __restrict__ at, uint32_t n, uint32_t n_docs,
                                          uint32_t* __restrict__ handles) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const mt_interval_add a = in[w];
    if (a.doc >= n_docs) {
        handles[w] = MT_REF_NONE;
        return;
    }
    mt_interval* iv = g.ivs + (size_t)a.doc * g.ivcap;
    mt_ref* tab = g.refs + (size_t)a.doc * 2 * g.refcap;
    uint32_t h = MT_REF_FULL;
    for (uint32_t s = 0; s < g.ivcap; s++) {
        if (iv[s].live == 0u && atomicCAS(&iv[s].live, 0u, 1u) == 0u) {
            h = s;
            break;
        }
    }
    if (h == MT_REF_FULL) {
        handles[w] = h;
        return;
    }
    // createSequenceInterval (intervalCollection.ts:207-243)
    uint32_t t0 = 0x10u, t1 = 0x20u;  // ReferenceType.RangeBegin / RangeEnd (ops.ts:11-12)
    if (a.interval_type == MT_INTERVAL_NEST) {
        t0 = 0x2u;  // NestBegin / NestEnd (ops.ts:9-10)
        t1 = 0x4u;
    }
    if (a.interval_type & MT_INTERVAL_SLIDE_ON_REMOVE) {
        t0 |= MT_REF_SLIDE_ON_REMOVE;
        t1 |= MT_REF_SLIDE_ON_REMOVE;
    }
    uint32_t got[2] = {MT_REF_FULL, MT_REF_FULL};
    bool attached = false;
    for (int k = 0; k < 2; k++) {
        const mt_pos_result p = at[2 * w + k];
        const bool on = (k ? a.end : a.start) >= 0 && p.ordinal >= 0;
        const uint32_t fl = MT_RF_LIVE | (on ? MT_RF_PENDING : 0u) | ((k ? t1 : t0) & MT_RF_TYPE);
        for (uint32_t s = 0; s < g.refcap; s++) {
            if (tab[s].flags == 0u && atomicCAS(&tab[s].flags, 0u, fl) == 0u) {
                tab[s].ord = on ? p.ordinal : -1;
                tab[s].off = on ? (uint32_t)p.offset : 0u;
                tab[s].rlen = on ? p.length : 0u;
                got[k] = s;
                break;
            }
        }
        if (got[k] == MT_REF_FULL) break;
        attached = attached || on;
    }
    if (got[1] == MT_REF_FULL) {  // hand back what was claimed
        if (got[0] != MT_REF_FULL) {
            tab[got[0]].ord = -1;
            tab[got[0]].off = 0u;
            tab[got[0]].rlen = 0u;
            __threadfence();
            atomicExch(&tab[got[0]].flags, 0u);
        }
        iv[h].live = 0u;
        handles[w] = MT_REF_FULL;
        return;
    }
    iv[h].start = got[0];
    iv[h].end = got[1];
    iv[h].type = (uint32_t)a.interval_type | ((uint32_t)a.collection << 16);
    atomicAdd(&g.ivn[a.doc], 1u);
    atomicAdd(&g.refn[a.doc], 2u);
    if (attached) {
        atomicOr(&g.refq[a.doc], MT_REFQ_DIRTY);
        atomicOr(&g.sc[a.doc].wide, MT_WIDE_LDS | MT_WIDE_REFS);
    }
    handles[w] = h;
}

extern "C" hipError_t mt_launch_intervals_claim(const mt_gstate* g, const mt_interval_add* in, const mt_pos_result* at,
                                                uint32_t n, uint32_t n_docs, uint32_t* handles, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_intervals_claim_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, in, at, n, n_docs, handles);
    return hipGetLastError();
}

// mt_intervals_remove: one wave per (document, start, end).  removeInterval (intervalCollection.ts:
// 330-336) removes the node whose key compares equal to the transient interval, endpoint by endpoint
// (SequenceInterval.compare, :140-147): the live entry of the lowest handle whose two ends equal
// getContainingSegment(start) / (end) in (ordinal, raw offset).  Its two references stay live, as the
// reference never calls removeLocalReference for them.
__global__ __launch_bounds__(64) void mt_intervals_release_kernel(mt_gstate g, const mt_interval_query* __restrict__ q,
                                                                  uint32_t nq, uint32_t n_docs,
                                                                  uint32_t* __restrict__ removed) {
    const uint32_t w = blockIdx.x;
    if (w >= nq) return;
    const int lane = lane_id();
    const mt_interval_query qq = q[w];
    const uint32_t d = qq.doc;
    uint32_t ans = MT_REF_NONE;
    if (d < n_docs && g.ivn[d] != 0) {
        End qs, qe;
        resolve2(g, d, qq.start, qq.end, qs, qe);
        mt_interval* iv = g.ivs + (size_t)d * g.ivcap;
        const mt_ref* __restrict__ tab = g.refs + (size_t)d * 2 * g.refcap;
        for (uint32_t base = 0; base < g.ivcap && ans == MT_REF_NONE; base += 64) {
            const uint32_t h = base + lane;
            bool hit = false;
            if (h < g.ivcap) {
                const mt_interval x = iv[h];
                if (x.live && (x.type >> 16) == qq.collection)
                    hit = cmp(end_of(tab, x.start, g.refcap), qs) == 0 && cmp(end_of(tab, x.end, g.refcap), qe) == 0;
            }
            uint64_t m = wave_ballot(hit);
            while (m && ans == MT_REF_NONE) {  // (another removal of this batch may take the entry first)
                const int l = first_lane(m);
                int took = 0;
                if (lane == l) took = atomicCAS(&iv[h].live, 1u, 0u) == 1u;
                took = __shfl(took, l, 64);
                if (took) ans = base + (uint32_t)l;
                m &= m - 1;
            }
        }
        if (ans != MT_REF_NONE && lane == 0) atomicSub(&g.ivn[d], 1u);
    }
    if (lane == 0) removed[w] = ans;
}

extern "C" hipError_t mt_launch_intervals_release(const mt_gstate* g, const mt_interval_query* q, uint32_t n,
                                                  uint32_t n_docs, uint32_t* removed, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_intervals_release_kernel, dim3(n), dim3(64), 0, st, *g, q, n, n_docs, removed);
    return hipGetLastError();
}

// the interval tables of documents ids[0..n) are freed (mt_docs_load; ids == nullptr: of documents
// 0..n-1): one wave per document
__global__ __launch_bounds__(64) void mt_intervals_free_docs_kernel(mt_gstate g, const uint32_t* __restrict__ ids,
                                                                    uint32_t n, uint32_t n_docs) {
    if (blockIdx.x >= n) return;
    const uint32_t d = ids ? ids[blockIdx.x] : blockIdx.x;
    if (d >= n_docs) return;
    for (uint32_t s = threadIdx.x; s < g.ivcap; s += 64) g.ivs[(size_t)d * g.ivcap + s] = mt_interval{0u, 0u, 0u, 0u};
    if (threadIdx.x == 0) g.ivn[d] = 0;
}

extern "C" hipError_t mt_launch_intervals_free_docs(const mt_gstate* g, const uint32_t* ids, uint32_t n, uint32_t n_docs,
                                                    hipStream_t st) {
    if (n == 0 || !g->ivs) return hipSuccess;
    hipLaunchKernelGGL(mt_intervals_free_docs_kernel, dim3(n), dim3(64), 0, st, *g, ids, n, n_docs);
    return hipGetLastError();
}

// mt_intervals_positions, after mt_refs_resolve_kernel answered every reference of the asked
// documents (g.refpos): one thread per (asked document, handle) picks its two ends' toPosition()
__global__ void mt_intervals_gather_kernel(mt_gstate g, const uint32_t* __restrict__ docs, uint32_t n, uint32_t n_docs,
                                           mt_interval_pos* __restrict__ out) {
    const uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= (uint64_t)n * g.ivcap) return;
    const uint32_t d = docs[w / g.ivcap], h = (uint32_t)(w % g.ivcap);
    mt_interval_pos r{-1, -1, 0, 0, 0u, MT_REF_NONE, MT_REF_NONE};
    if (d < n_docs) {
        const mt_interval x = g.ivs[(size_t)d * g.ivcap + h];
        if (x.live) {
            r.interval_type = (uint16_t)(x.type & 0xFFFFu);
            r.collection = (uint16_t)(x.type >> 16);
            r.live = 1u;
            r.start_ref = x.start;
            r.end_ref = x.end;
            if (x.start < g.refcap) r.start = g.refpos[(size_t)d * g.refcap + x.start].position;
            if (x.end < g.refcap) r.end = g.refpos[(size_t)d * g.refcap + x.end].position;
        }
    }
    out[w] = r;
}

extern "C" hipError_t mt_launch_intervals_gather(const mt_gstate* g, const uint32_t* docs, uint32_t n, uint32_t n_docs,
                                                 mt_interval_pos* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    const uint64_t tot = (uint64_t)n * g->ivcap;
    hipLaunchKernelGGL(mt_intervals_gather_kernel, dim3((uint32_t)((tot + 255) / 256)), dim3(256), 0, st, *g, docs, n,
                       n_docs, out);
    return hipGetLastError();
}
