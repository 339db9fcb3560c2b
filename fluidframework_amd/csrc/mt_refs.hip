// mt_refs.hip -- local references (include/mtgpu.h "local references"): the per-document table of
// (segment ordinal, offset) pairs, the tracker that folds the document's delta / maintenance
// events into it, and the resolve to local positions.  Nothing here runs inside an apply.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mtgpu.h"
#include "mt_launch.h"
#include "mt_state.h"
#include "mt_wave.h"

namespace {

// an entry that sits in its segment's LocalReferenceCollection (mt_state.h mt_ref)
MT_DEV bool in_coll(const mt_ref& e) {
    return (e.flags & MT_RF_GHOST) ||
           ((e.flags & MT_RF_LIVE) && !(e.flags & (MT_RF_LOOSE | MT_RF_PENDING)) && e.ord >= 0);
}
MT_DEV bool is_ref(const mt_ref& e) { return (e.flags & MT_RF_LIVE) && !(e.flags & (MT_RF_LOOSE | MT_RF_PENDING)) && e.ord >= 0; }

// One document's table staged in LDS; every method is called by the whole wave with uniform
// arguments.  Lanes own entries lane, lane + 64, ...; a method that reads other lanes' entries
// starts with a wave_sync and one that writes ends with one.
struct Tab {
    mt_ref* t;
    int T, P, lane;  // entries, of which references (the ghosts follow)
    uint32_t dropped = 0;  // ghosts that found no room (uniform)
    // refsByOffset.length of segment L's collection, -1: it has none
    MT_DEV int coll_rlen(int L) const {
        int r = -1;
        for (int i = lane; i < T; i += 64)
            if (in_coll(t[i]) && t[i].ord == L) r = max(r, (int)t[i].rlen);
        return wave_max(r);
    }
    // references in segment L's collection at offsets >= from
    MT_DEV int refs_on(int L, uint32_t from) const {
        int c = 0;
        for (int i = lane; i < T; i += 64)
            if (is_ref(t[i]) && t[i].ord == L && t[i].off >= from) c++;
        return wave_sum(c);
    }
    MT_DEV void set_rlen(int L, uint32_t r) {
        for (int i = lane; i < T; i += 64)
            if (in_coll(t[i]) && t[i].ord == L) t[i].rlen = r;
        wave_sync();
    }
    // segment `ord` keeps a collection without references (dropped, and counted, when the ghosts'
    // half is full)
    MT_DEV void make_ghost(int ord, uint32_t rlen) {
        bool placed = false;
        for (int base = P; base < T && !placed; base += 64) {
            const int i = base + lane;
            const uint64_t m = wave_ballot(i < T && t[i].flags == 0u);
            if (m) {
                if (lane == first_lane(m)) t[i] = mt_ref{ord, 0u, MT_RF_GHOST, rlen};
                placed = true;
            }
        }
        if (!placed) dropped++;
        wave_sync();
    }
    // a ghost beside references of its segment carries nothing they do not: its slot is free again
    MT_DEV void reap(int L) {
        if (refs_on(L, 0u) == 0) return;
        for (int i = lane; i < T; i += 64)
            if ((t[i].flags & MT_RF_GHOST) && t[i].ord == L) t[i] = mt_ref{-1, 0u, 0u, 0u};
        wave_sync();
    }
    // ordinals >= from move by delta (leaves linked or unlinked before them)
    MT_DEV void shift(int from, int delta) {
        for (int i = lane; i < T; i += 64)
            if (t[i].flags != 0u && t[i].ord >= from) t[i].ord += delta;
        wave_sync();
    }

    // Entries added or removed since the last fold (mt_refs_add / mt_refs_remove), in slot order:
    // addLocalRef creates the segment's collection at its cachedLength when it has none and grows
    // refsByOffset to offset + 1 (localReference.ts:212-225); removeLocalRef leaves the collection.
    MT_DEV void settle() {
        for (int s = 0; s < P; s++) {
            const mt_ref e = t[s];  // (uniform)
            if (e.flags & MT_RF_ZOMBIE) {
                const int r = coll_rlen(e.ord);
                if (lane == 0) t[s] = mt_ref{-1, 0u, 0u, 0u};
                wave_sync();
                if (r < 0) make_ghost(e.ord, e.rlen);
            } else if (e.flags & MT_RF_PENDING) {
                const int r0 = coll_rlen(e.ord);
                const uint32_t r = r0 < 0 ? max(e.rlen, e.off + 1u) : max((uint32_t)r0, e.off + 1u);
                if (lane == 0) {
                    t[s].flags = e.flags & ~MT_RF_PENDING;
                    t[s].rlen = r;
                }
                wave_sync();
                set_rlen(e.ord, r);
                reap(e.ord);
            }
        }
    }

    // BaseSegment.splitAt -> LocalReferenceCollection.split (mergeTree.ts:562-564, localReference.ts:283-301)
    MT_DEV void split(int L, uint32_t len1) {
        const int r = coll_rlen(L);
        const int all = r >= 0 ? refs_on(L, 0u) : 0;
        const int moved = all ? refs_on(L, len1) : 0;
        shift(L + 1, 1);
        if (!all) return;  // no collection, or an empty one: nothing is spliced
        const uint32_t r1 = min((uint32_t)r, len1), r2 = (uint32_t)r > len1 ? (uint32_t)r - len1 : 0u;
        for (int i = lane; i < T; i += 64) {
            if (!in_coll(t[i]) || t[i].ord != L) continue;
            if (is_ref(t[i]) && t[i].off >= len1) {
                t[i].ord = L + 1;
                t[i].off -= len1;
                t[i].rlen = r2;
            } else {
                t[i].rlen = r1;
            }
        }
        wave_sync();
        if (moved == 0) make_ghost(L + 1, r2);
        if (moved == all && coll_rlen(L) < 0) make_ghost(L, r1);
    }

    // TextSegment.append -> LocalReferenceCollection.append (textSegment.ts:74-81, localReference.ts:128-135,
    // 268-281): segment L + 1 (len2) joins segment L (len1 before it grows)
    MT_DEV void append(int L, uint32_t len1) {
        const int r2 = coll_rlen(L + 1);
        const int n2 = r2 >= 0 ? refs_on(L + 1, 0u) : 0;
        int r1 = coll_rlen(L);
        if (n2 && r1 < 0) r1 = (int)len1;  // a new collection, at the segment's length before the append
        for (int i = lane; i < T; i += 64) {
            if (t[i].flags == 0u || t[i].ord != L + 1) continue;
            if (n2 && is_ref(t[i])) {
                t[i].ord = L;
                t[i].off += (uint32_t)r1;  // this.refsByOffset.length, stale or not
            } else if (t[i].flags & MT_RF_GHOST) {
                t[i] = mt_ref{-1, 0u, 0u, 0u};
            }
        }
        wave_sync();
        if (n2) {
            set_rlen(L, (uint32_t)(r1 + r2));
            reap(L);
        }
        shift(L + 2, -1);
    }

    // zamboni unlinks segment L (mergeTree.ts:1310-1317)
    MT_DEV void unlink(int L) {
        for (int i = lane; i < T; i += 64) {
            if (t[i].flags == 0u || t[i].ord != L) continue;
            if (t[i].flags & MT_RF_LIVE) {
                t[i].ord = -1;  // (off stays: a detached reference keeps its raw offset, which
                                // LocalReference.compare still reads -- mt_intervals.hip)
            } else {
                t[i] = mt_ref{-1, 0u, 0u, 0u};
            }
        }
        wave_sync();
        shift(L + 1, -1);
    }

    // markRangeRemoved removed segment L (mergeTree.ts:2639-2643, 2671-2696); the callback's slide
    // target is segment tgt (-1: none) of cachedLength tlen
    MT_DEV void removed(int L, int tgt, uint32_t tlen, bool after) {
        const int saved = refs_on(L, 0u);  // (savedLocalRefs holds only collections that are not empty)
        int slid = 0;
        for (int i = lane; i < T; i += 64) {
            if (t[i].flags == 0u || t[i].ord != L) continue;
            if (t[i].flags & MT_RF_GHOST) {
                t[i] = mt_ref{-1, 0u, 0u, 0u};  // segment.localRefs = undefined
            } else if (saved && is_ref(t[i])) {
                if (tgt >= 0 && (t[i].flags & MT_REF_SLIDE_ON_REMOVE)) {
                    t[i].ord = -2;  // (joins the target below, once its collection's length is known)
                    slid++;
                } else if (tgt < 0 && (t[i].flags & MT_RF_AFTER)) {
                    t[i].flags |= MT_RF_LOOSE;  // clear() skips the `after` lists
                } else {
                    t[i].ord = -1;  // lref.segment = undefined: the offset stays (localReference.ts:193, 318)
                }
            }
        }
        wave_sync();
        if (!saved || tgt < 0) return;
        slid = wave_sum(slid);
        int r = coll_rlen(tgt);
        const bool fresh = r < 0;
        if (fresh) r = (int)tlen;  // new LocalReferenceCollection(refSegment)
        // addBeforeTombstones assigns refsByOffset[0], addAfterTombstones refsByOffset[cachedLength - 1]
        if (slid) r = max(r, after ? (int)tlen : 1);
        for (int i = lane; i < T; i += 64) {
            if (t[i].flags == 0u || t[i].ord != -2) continue;
            t[i].ord = tgt;
            t[i].off = after ? tlen - 1u : 0u;
            t[i].rlen = (uint32_t)r;
            t[i].flags = (t[i].flags & ~(MT_RF_BEFORE | MT_RF_AFTER)) | (after ? MT_RF_AFTER : MT_RF_BEFORE);
        }
        wave_sync();
        set_rlen(tgt, (uint32_t)r);
        if (fresh && !slid) make_ghost(tgt, (uint32_t)r);
        if (slid) reap(tgt);
    }
};

}  // namespace

// The tracker: one wave per document, its table in LDS, one entry per lane (64-entry chunks),
// folding the document's event rows [refcur, evn) in firing order.  Every row is wave-uniform (one
// load, by a uniform index).  Rules, with the reference's lines, in include/mtgpu.h.
__global__ __launch_bounds__(64) void mt_refs_track_kernel(mt_gstate g, uint32_t n_docs) {
    extern __shared__ mt_ref lds_tab[];
    const uint32_t d = blockIdx.x;
    if (d >= n_docs) return;
    const int lane = lane_id();
    const uint32_t evn = min(g.evn[d], g.evcap);  // (a halted document's count may pass the capacity)
    const uint32_t cur = min(g.refcur[d], evn);
    const bool dirty = (g.refq[d] & MT_REFQ_DIRTY) != 0;
    if (g.refn[d] != 0 && (cur < evn || dirty)) {
        const int T = 2 * (int)g.refcap;
        mt_ref* gt = g.refs + (size_t)d * T;
        Tab tb{lds_tab, T, (int)g.refcap, lane};
        for (int i = lane; i < T; i += 64) tb.t[i] = gt[i];
        wave_sync();
        if (dirty) tb.settle();
        const mt_event* __restrict__ ev = g.ev + (size_t)d * g.evcap;
        int t_ord = -1, a_leaf = -1;
        uint32_t t_len = 0, t_after = 0, a_grown = 0;
        for (uint32_t k = cur; k < evn; k++) {
            const mt_event& e = ev[__builtin_amdgcn_readfirstlane(k)];
            const int op = e.op, L = e.leaf;
            const uint32_t ef = e.flags, len = e.len;
            if (op == MT_EV_INSERT) {
                if (L >= 0) tb.shift(L, 1);
            } else if (op == MT_EV_SPLIT) {
                if (ef & MT_EVF_FIRST) tb.split(L, len);  // (the second half's row: L + 1, nothing more)
            } else if (op == MT_EV_APPEND) {
                if (ef & MT_EVF_FIRST) {
                    a_leaf = L;
                    a_grown = len;
                } else if (L == a_leaf + 1) {  // (else: a callback cut short by a full buffer)
                    tb.append(a_leaf, a_grown - len);
                }
            } else if (op == MT_EV_UNLINK) {
                tb.unlink(L);
            } else if (op == MT_EV_REMOVE) {
                if (ef & MT_EVF_FIRST) {
                    const uint64_t t = e.pad2;
                    t_ord = MT_EVT_ORDINAL(t);
                    t_len = MT_EVT_LENGTH(t);
                    t_after = MT_EVT_AFTER(t);
                }
                if (!(ef & MT_EVF_EMPTY) && L >= 0) tb.removed(L, t_ord, t_len, t_after != 0);
            }
        }
        int used = 0;
        for (int i = lane; i < T; i += 64) {
            gt[i] = tb.t[i];
            used += tb.t[i].flags != 0u;
        }
        used = wave_sum(used);
        if (lane == 0) {
            g.refn[d] = (uint32_t)used;
            g.refq[d] &= ~MT_REFQ_DIRTY;
            g.refdrop[d] += tb.dropped;
        }
    }
    if (lane == 0) g.refcur[d] = evn;
}

extern "C" hipError_t mt_launch_refs_track(const mt_gstate* g, uint32_t n_docs, hipStream_t st) {
    if (n_docs == 0 || !g->refs || !g->ev) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_track_kernel, dim3(n_docs), dim3(64), 2 * g->refcap * sizeof(mt_ref), st, *g, n_docs);
    return hipGetLastError();
}

// mt_refs_add, after mt_resolve_kernel answered getContainingSegment(pos) of the local view per entry:
// one thread per entry claims a free slot of its document's table and marks the document.  The
// entry is pending (rlen: its segment's cachedLength) until the next fold settles it.
__global__ void mt_refs_claim_kernel(mt_gstate g, const mt_ref_add* __restrict__ in,
                                     const mt_pos_result* __restrict__ at, uint32_t n, uint32_t n_docs,
                                     uint32_t* __restrict__ handles) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const mt_ref_add a = in[w];
    const mt_pos_result p = at[w];
    uint32_t h = MT_REF_NONE;
    if (a.doc < n_docs && a.pos >= 0 && p.ordinal >= 0) {
        h = MT_REF_FULL;
        mt_ref* tab = g.refs + (size_t)a.doc * 2 * g.refcap;
        const uint32_t fl = MT_RF_LIVE | MT_RF_PENDING | (a.ref_type & MT_RF_TYPE);
        for (uint32_t s = 0; s < g.refcap; s++) {
            if (tab[s].flags == 0u && atomicCAS(&tab[s].flags, 0u, fl) == 0u) {
                tab[s].ord = p.ordinal;
                tab[s].off = (uint32_t)p.offset;
                tab[s].rlen = p.length;
                atomicAdd(&g.refn[a.doc], 1u);
                atomicOr(&g.refq[a.doc], MT_REFQ_DIRTY);
                atomicOr(&g.sc[a.doc].wide, MT_WIDE_LDS | MT_WIDE_REFS);
                h = s;
                break;
            }
        }
    }
    handles[w] = h;
}

extern "C" hipError_t mt_launch_refs_claim(const mt_gstate* g, const mt_ref_add* in, const mt_pos_result* at, uint32_t n,
                                           uint32_t n_docs, uint32_t* handles, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_claim_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, in, at, n, n_docs, handles);
    return hipGetLastError();
}

// mt_refs_remove: a reference in a collection stays as a zombie until the next fold (its segment's
// collection outlives it); any other is freed at once
__global__ void mt_refs_release_kernel(mt_gstate g, const uint32_t* __restrict__ docs, const uint32_t* __restrict__ handles,
                                       uint32_t n, uint32_t n_docs) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint32_t d = docs[w], h = handles[w];
    if (d >= n_docs || h >= g.refcap) return;
    mt_ref* e = g.refs + (size_t)d * 2 * g.refcap + h;
    const uint32_t fl = e->flags;
    if (!(fl & MT_RF_LIVE)) return;
    const bool coll = !(fl & (MT_RF_LOOSE | MT_RF_PENDING)) && e->ord >= 0;
    if (atomicCAS(&e->flags, fl, coll ? MT_RF_ZOMBIE : 0u) == fl && coll) atomicOr(&g.refq[d], MT_REFQ_DIRTY);
}

extern "C" hipError_t mt_launch_refs_release(const mt_gstate* g, const uint32_t* docs, const uint32_t* handles, uint32_t n,
                                             uint32_t n_docs, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_release_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, docs, handles, n, n_docs);
    return hipGetLastError();
}

// the references of documents ids[0..n) are freed (mt_docs_load): one wave per document
__global__ __launch_bounds__(64) void mt_refs_free_docs_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                               uint32_t n_docs) {
    if (blockIdx.x >= n) return;
    const uint32_t d = ids[blockIdx.x];
    if (d >= n_docs) return;
    const uint32_t T = 2 * g.refcap;
    for (uint32_t s = threadIdx.x; s < T; s += 64) g.refs[(size_t)d * T + s] = mt_ref{-1, 0u, 0u, 0u};
    if (threadIdx.x == 0) {
        g.refn[d] = 0;
        g.refq[d] = 0;
        g.refdrop[d] = 0;
        g.refcur[d] = g.evn ? min(g.evn[d], g.evcap) : 0u;
    }
}

extern "C" hipError_t mt_launch_refs_free_docs(const mt_gstate* g, const uint32_t* ids, uint32_t n, uint32_t n_docs,
                                               hipStream_t st) {
    if (n == 0 || !g->refs) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_free_docs_kernel, dim3(n), dim3(64), 0, st, *g, ids, n, n_docs);
    return hipGetLastError();
}

// mt_refs_positions, step 1: mark the queried documents
__global__ void mt_refs_mark_kernel(mt_gstate g, const uint32_t* __restrict__ docs, uint32_t n, uint32_t n_docs) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w < n && docs[w] < n_docs) atomicOr(&g.refq[docs[w]], MT_REFQ_ASKED);
}

// step 2: one wave per queried document resolves its live references, one per lane (looping past
// 64), in one pass per lane chunk over the document's leaves in 64-leaf chunks that carries the
// local view's running prefix; a lane takes its answer when the chunk holding its ordinal passes:
// position = getPosition(segment) + (segment removed ? 0 : offset) (LocalReference.toPosition /
// getOffset, localReference.ts:63-69, 109-114; a pending local removal, removedSeq -1, counts).
__global__ __launch_bounds__(64) void mt_refs_resolve_kernel(mt_gstate g, uint32_t n_docs) {
    const uint32_t d = blockIdx.x;
    if (d >= n_docs || !(g.refq[d] & MT_REFQ_ASKED)) return;
    const int lane = lane_id();
    const int n = g.sc[d].nseg;
    const size_t so = (size_t)d * g.segcap;
    const mt_ref* tab = g.refs + (size_t)d * 2 * g.refcap;
    mt_ref_pos* res = g.refpos + (size_t)d * g.refcap;
    for (uint32_t rb = 0; rb < g.refcap; rb += 64) {
        const uint32_t slot = rb + lane;
        mt_ref r{-1, 0u, 0u, 0u};
        if (slot < g.refcap) r = tab[slot];
        const bool want = (r.flags & MT_RF_LIVE) && r.ord >= 0 && r.ord < n;
        mt_ref_pos ans{-1, (r.flags & MT_RF_LIVE) ? -1 : MT_REF_BAD_HANDLE, 0u};
        const int last = wave_max(want ? r.ord : -1);  // leaves past it answer nobody
        int carry = 0;
        for (int base = 0; base <= last; base += 64) {
            const int i = base + lane;
            const int rm = (i < n && (g.flags[so + i] & MT_SF_REMOVED)) ? 1 : 0;
            const int ll = (i < n && !rm) ? (int)g.len[so + i] : 0;
            const int incl = carry + wave_incl_scan(ll);
            const bool in = want && r.ord >= base && r.ord < base + 64;
            const int src = in ? r.ord - base : 0;
            const int before = __shfl(incl - ll, src, 64);
            const int srm = __shfl(rm, src, 64);
            if (in) {
                ans.offset = srm ? 0u : r.off;
                ans.position = before + (int)ans.offset;
                ans.ordinal = r.ord;
            }
            carry = wave_last(incl);
        }
        if (slot < g.refcap) res[slot] = ans;
    }
    if (lane == 0) g.refq[d] &= ~MT_REFQ_ASKED;
}

// step 3: one thread per query picks its reference's answer
__global__ void mt_refs_gather_kernel(mt_gstate g, const uint32_t* __restrict__ docs, const uint32_t* __restrict__ handles,
                                      uint32_t n, uint32_t n_docs, mt_ref_pos* __restrict__ out) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint32_t d = docs[w], h = handles[w];
    mt_ref_pos r{-1, MT_REF_BAD_HANDLE, 0u};
    if (d < n_docs && h < g.refcap) r = g.refpos[(size_t)d * g.refcap + h];
    out[w] = r;
}

// steps 1 and 2 alone: g.refpos of documents docs[0..n) answers for every reference they hold
// (mt_intervals_positions gathers from it)
extern "C" hipError_t mt_launch_refs_resolve_docs(const mt_gstate* g, const uint32_t* docs, uint32_t n, uint32_t n_docs,
                                                  hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, docs, n, n_docs);
    hipLaunchKernelGGL(mt_refs_resolve_kernel, dim3(n_docs), dim3(64), 0, st, *g, n_docs);
    return hipGetLastError();
}

extern "C" hipError_t mt_launch_refs_positions(const mt_gstate* g, const uint32_t* docs, const uint32_t* handles, uint32_t n,
                                               uint32_t n_docs, mt_ref_pos* out, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_mark_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, docs, n, n_docs);
    hipLaunchKernelGGL(mt_refs_resolve_kernel, dim3(n_docs), dim3(64), 0, st, *g, n_docs);
    hipLaunchKernelGGL(mt_refs_gather_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, docs, handles, n, n_docs, out);
    return hipGetLastError();
}

// mt_refs_insert_local, after the resolve: one thread per record lowers it to MT_OP_INSERT_AT at its
// reference's leaf (ordinal, getOffset) and answers the reference's local position.  The record of a
// detached reference or of a handle that names none becomes a message without an op at the
// document's own window (seq = currentSeq, msn = minSeq): it applies as nothing at all.
__global__ void mt_refs_stamp_kernel(mt_gstate g, const uint32_t* __restrict__ docs, const mt_ref_pos* __restrict__ at,
                                     mt_op_rec* __restrict__ ops, uint32_t n, uint32_t n_docs,
                                     int32_t* __restrict__ positions) {
    const uint32_t w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= n) return;
    const uint32_t d = docs[w];
    const mt_ref_pos r = at[w];
    mt_op_rec o = ops[w];
    if (d < n_docs && r.ordinal >= 0 && r.position >= 0) {
        o.type = MT_OP_INSERT_AT;
        o.pos1 = r.ordinal;
        o.pos2 = (int32_t)r.offset;
        positions[w] = r.position;
    } else {
        const mt_doc_scalars& sc = g.sc[d < n_docs ? d : 0];
        o.seq = sc.cur_seq;
        o.ref_seq = sc.cur_seq;
        o.msn = sc.min_seq;
        o.type = MT_OP_NOOP;
        o.flags = 0;
        o.pos1 = o.pos2 = 0;
        o.payload_len = 0;
        positions[w] = r.ordinal == MT_REF_BAD_HANDLE ? MT_REF_BAD_HANDLE : -1;
    }
    ops[w] = o;
}

extern "C" hipError_t mt_launch_refs_stamp(const mt_gstate* g, const uint32_t* docs, const mt_ref_pos* at, mt_op_rec* ops,
                                           uint32_t n, uint32_t n_docs, int32_t* positions, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_refs_stamp_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *g, docs, at, ops, n, n_docs,
                       positions);
    return hipGetLastError();
}
