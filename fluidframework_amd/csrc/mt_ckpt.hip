// mt_ckpt.hip -- document checkpoints on the device: sizing, the gather of a document's at-rest state
// into a blob (pack) and the reverse scatter into a slot (unpack).  The format and the list of
// sections are mt_ckpt.h's (mt_ckpt_walk); nothing here decides a size.
//
// Both copies are memory bound.  Between launches every array of a document is compact and in
// document order (mt_state.h), so a section is one contiguous range on both sides (the two halves of
// a wide segment's overlap row apart: 32 of every 64 bytes).  A section starts on a 16-byte boundary
// in the blob; where the engine's row does too (the per-segment arrays of an engine whose
// seg_capacity is a multiple of 16, the text, the pool rows) a lane moves 16 bytes per instruction
// and only the section's last partial vector goes byte by byte; a row that is not (the heap from
// entry 1 on, an odd capacity, an editing document's mt_loc: 540 bytes per slot) is copied at the widest
// unit both sides share.
//
// Workgroup: 256 threads per document, `parts` workgroups per document (grid.y).  A document of a few
// KB has ~25 short sections and is bound by their latency, not by lanes: the four waves each take a
// quarter of every section's vectors, and 100 K such documents fill the device by themselves.  A
// 65472-segment document with a 64 MiB arena is 70 MB: one workgroup would copy it alone on one CU,
// so the host asks for one part per 64 KiB of the largest document (at most 64) and the parts share
// every section's vectors.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mt_ckpt.h"
#include "mt_launch.h"
#include "mt_wave.h"

namespace {

constexpr uint32_t kCkThreads = 256;

// dst[0..n) = src[0..n) by the `nth` threads that share the copy (tid: this one); every branch is
// uniform over them.  Vectors of 16 bytes when the two addresses agree mod 16 (a head of up to 15
// bytes and a tail byte by byte), words when they agree mod 4, else bytes.
__device__ __forceinline__ void ck_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, uint64_t n,
                                        uint32_t tid, uint32_t nth) {
    if (n == 0) return;
    const uintptr_t a = (uintptr_t)dst, b = (uintptr_t)src;
    const uint32_t unit = ((a ^ b) & 15) == 0 ? 16u : ((a ^ b) & 3) == 0 ? 4u : 1u;
    uint64_t head = (unit - (a & (unit - 1))) & (unit - 1);
    if (head > n) head = n;
    const uint64_t nv = unit == 1 ? 0 : (n - head) / unit, tail = head + nv * unit;  // (bytes: all of it is tail)
    for (uint64_t i = tid; i < head; i += nth) dst[i] = src[i];
    if (unit == 16) {
        const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src + head);
        uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst + head);
        for (uint64_t v = tid; v < nv; v += nth) d4[v] = s4[v];
    } else if (unit == 4) {
        const uint32_t* __restrict__ s1 = reinterpret_cast<const uint32_t*>(src + head);
        uint32_t* __restrict__ d1 = reinterpret_cast<uint32_t*>(dst + head);
        for (uint64_t v = tid; v < nv; v += nth) d1[v] = s1[v];
    }
    for (uint64_t i = tail + tid; i < n; i += nth) dst[i] = src[i];
}

// Where section `id` of the document in slot d lives in the engine (its first byte).  Null: the overlap
// halves (not one range there), an editing client's sections (the kernels of their own below: ck_loc_ptr),
// and the sections of the documents the host does not admit -- the label cache, references, intervals
// (mt_engine.cpp ckpt_supported): they are never copied.  `half`: the arena half the text is read from /
// written to.
__device__ __forceinline__ uint8_t* ck_engine_ptr(const mt_gstate& g, uint32_t d, uint32_t half, int id) {
    const size_t so = (size_t)d * g.segcap;
    auto p = [](auto* q) { return reinterpret_cast<uint8_t*>(q); };
    switch (id) {
        case CK_SEQ: return p(g.seq + so);
        case CK_RSEQ: return p(g.rseq + so);
        case CK_LEN: return p(g.len + so);
        case CK_TOFF: return p(g.toff + so);
        case CK_OVL: return p(g.ovl + so);
        case CK_PROPS: return p(g.props + so);
        case CK_CLIENT: return p(g.client + so);
        case CK_RCLIENT: return p(g.rclient + so);
        case CK_FLAGS: return p(g.flags + so);
        case CK_CHI: return p(g.chi + so);
        case CK_PH: return p(g.ph + so);
        case CK_PXL: return p(g.pxl + so);
        case CK_PXH: return p(g.pxh + so);
        case CK_PXX: return p(g.pxx + 4 * so);
        case CK_LBCNT: return p(g.lbcnt + (size_t)d * g.lbcap);
        case CK_LBSCOUR: return p(g.lbscour + (size_t)d * g.lbcap);
        case CK_IB1: case CK_IB2: case CK_IB3: case CK_IB4: case CK_IB5: case CK_IB6:
            return p(g.ibcnt + ((size_t)d * (MT_MAXLEV - 1) + (id - CK_IB1)) * g.ibcap);
        case CK_HSEQ: return p(g.hseq + (size_t)d * g.hcap + 1);
        case CK_HSLOT: return p(g.hslot + (size_t)d * g.hcap + 1);
        case CK_TEXT: return g.text + ((size_t)d * 2 + half) * g.textcap;
        default: return nullptr;
    }
}

// An editing client's sections (CK_LOC .. CK_RGP) have kernels of their own, launched only when a
// document of the call carries MT_CKF_LOC: inlined into the walk of the kernels above they cost every
// observer document registers and time (DESIGN.md "Measurement").
// The pool rows of the document in slot d (MT_NO_ROW: none): read once per workgroup, before the walk.
struct CkRows {
    uint32_t big = MT_NO_ROW, gx = MT_NO_ROW, wx = MT_NO_ROW;
};
__device__ __forceinline__ CkRows ck_rows(const mt_gstate& g, uint32_t d, uint32_t flags) {
    CkRows r;
    if (flags & MT_CKF_BIG) r.big = g.locbig[d];
    if (flags & MT_CKF_GX) r.gx = g.locgx[d];
    if (flags & MT_CKF_WX) r.wx = g.locwx[d];
    return r;
}
// Where editing section `id` of the document in slot d lives (its first byte); null: a pool section of a
// document that holds no such row.  Its per-segment state lies in its big-pool row when it holds one, else
// in its own 1024-slot row; the section sizes (mt_ckpt_nloc) never pass the row that the flags name.
__device__ __forceinline__ uint8_t* ck_loc_ptr(const mt_gstate& g, uint32_t d, int id, uint32_t flags, const CkRows& rows) {
    auto p = [](auto* q) { return reinterpret_cast<uint8_t*>(q); };
    const bool big = (flags & MT_CKF_BIG) != 0;
    const size_t lo = big ? (size_t)rows.big * MT_LOC_BIGCAP : (size_t)d * MT_LOC_CAP;
    switch (id) {
        case CK_LOC: return p(g.loc + d);
        case CK_GM: return big && rows.big == MT_NO_ROW ? nullptr : p((big ? g.gmb : g.gm) + lo);
        case CK_PK: return big && rows.big == MT_NO_ROW ? nullptr : p((big ? g.pkb : g.pk) + lo);
        case CK_CT: return big && rows.big == MT_NO_ROW ? nullptr : p((big ? g.ctb : g.ct) + lo);
        case CK_LSQ: return big && rows.big == MT_NO_ROW ? nullptr : p((big ? g.lsqb : g.lsq) + lo);
        case CK_GMX: return rows.gx == MT_NO_ROW ? nullptr : p(g.gmx + (size_t)rows.gx * MT_LOC_BIGCAP * MT_LOC_GW);
        case CK_LOCX: return rows.gx == MT_NO_ROW ? nullptr : p(g.locx + rows.gx);
        case CK_PKW: return rows.wx == MT_NO_ROW ? nullptr : p(g.pkw + (size_t)rows.wx * MT_LOC_BIGCAP * MT_PKW_WORDS);
        case CK_RG: return p(g.rg + (size_t)d * MT_RG_RECS);
        case CK_RGP: return g.rgp + (size_t)d * MT_RG_BYTES;
        default: return nullptr;
    }
}

// The checkpoint header of the document in slot d as it stands: what decides every section's size.
// Called by every lane of one wave (the table counts are wave sums).
__device__ __forceinline__ mt_ckpt_dochdr ck_header(const mt_gstate& g, uint32_t d, int lane) {
    mt_ckpt_dochdr h{};
    h.sc = g.sc[d];
    h.sc.text_half = 0;
    // what the rows hold (a document halted over a capacity may count past it: the stores clamp too)
    h.sc.nseg = min(h.sc.nseg, (int32_t)g.segcap);
    h.sc.heap_n = min(h.sc.heap_n, (int32_t)g.hcap - 1);
    h.sc.nlev = min(h.sc.nlev, MT_MAXLEV);
    h.sc.nb[0] = min(h.sc.nb[0], (int32_t)g.lbcap);
    for (int l = 1; l < MT_MAXLEV; l++) h.sc.nb[l] = min(h.sc.nb[l], (int32_t)g.ibcap);
    h.sc.text_top = min(h.sc.text_top, (h.sc.wide & MT_WIDE_DOC) ? g.textcap / 2 : g.textcap);
    const mt_loc& lc = g.loc[d];
    if (lc.own >= 0) {
        // (a group row of a document that is not MT_WIDE_GROUPS, or a wide row of a narrow one, was never stored
        // into -- the document halted in the launch that was to take it there -- and is not read by its next
        // load either (mt_apply.hip load): it is not part of its state.  A wide document that halted in the very
        // launch that gave it its wide row saves that row as the pool held it: bytes of a halted document that
        // nothing reads, and the same bytes again after a restore.)
        h.flags = MT_CKF_LOC | (g.locbig[d] != MT_NO_ROW ? MT_CKF_BIG : 0u) |
                  (g.locgx[d] != MT_NO_ROW && (h.sc.wide & MT_WIDE_GROUPS) ? MT_CKF_GX : 0u) |
                  (g.locwx[d] != MT_NO_ROW && (h.sc.wide & MT_WIDE_DOC) ? MT_CKF_WX : 0u);
        h.rgn = min(lc.rgn, (uint32_t)MT_RG_RECS);
        h.rgpn = min(lc.rgpn, (uint32_t)MT_RG_BYTES);
    }
    if (g.refs && g.refn[d]) {
        const mt_ref* __restrict__ t = g.refs + (size_t)d * 2 * g.refcap;
        int used = 0;
        for (uint32_t i = lane; i < 2 * g.refcap; i += 64) used += t[i].flags != 0u;
        h.n_refs = (uint32_t)wave_sum(used);
        h.refdrop = g.refdrop[d];
    }
    if (g.ivs && g.ivn[d]) {
        const mt_interval* __restrict__ t = g.ivs + (size_t)d * g.ivcap;
        int used = 0;
        for (uint32_t i = lane; i < g.ivcap; i += 64) used += t[i].live != 0u;
        h.n_ivs = (uint32_t)wave_sum(used);
    }
    return h;
}

}  // namespace

// One wave per document: its checkpoint header (the host sums the sizes that follow from it, in 64 bits).
__global__ __launch_bounds__(64) void mt_ckpt_size_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                          mt_ckpt_dochdr* __restrict__ hdr) {
    const uint32_t w = blockIdx.x;
    if (w >= n) return;
    const mt_ckpt_dochdr h = ck_header(g, ids[w], lane_id());
    if (lane_id() == 0) hdr[w] = h;
}

// One or more workgroups per document (grid.y parts): every section gathered to out + off[w].
// hdr: the sizing kernel's, nothing having changed the documents since.
__global__ __launch_bounds__(256) void mt_ckpt_pack_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                           const mt_ckpt_dochdr* __restrict__ hdr,
                                                           const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
    const uint32_t w = blockIdx.x;
    if (w >= n) return;
    const uint32_t d = ids[w];
    const uint32_t tid = blockIdx.y * kCkThreads + threadIdx.x, nth = gridDim.y * kCkThreads;
    const mt_ckpt_dochdr h = hdr[w];
    const uint32_t half = g.sc[d].text_half;
    uint8_t* __restrict__ doc = out + off[w];
    if (tid < sizeof(mt_ckpt_dochdr) / 16) reinterpret_cast<uint4*>(doc)[tid] = reinterpret_cast<const uint4*>(hdr + w)[tid];
    const size_t so = (size_t)d * g.segcap;
    const uint32_t ns = mt_ckpt_nseg(h);
    mt_ckpt_walk(h, [&](int id, uint64_t o, uint64_t b) {
        uint8_t* __restrict__ dst = doc + o;
        for (uint64_t q = b + tid; q < mt_ckpt_align(b); q += nth) dst[q] = 0;  // the padding
        if (b == 0) return;
        if (id == CK_OVX0 || id == CK_OVX1) {  // 32 of a segment's 64 bytes: two vectors each
            const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(g.ovx + MT_OVX_WORDS * so) + (id == CK_OVX1 ? 2 : 0);
            uint4* __restrict__ d4 = reinterpret_cast<uint4*>(dst);
            for (uint64_t v = tid; v < 2ull * ns; v += nth) d4[v] = s4[(v >> 1) * 4 + (v & 1)];
        } else if (uint8_t* src = ck_engine_ptr(g, d, half, id)) {
            ck_copy(dst, src, b, tid, nth);
        }
    });
}

// The reverse: the checked document at in + off[w] into slot ids[w].  The host took the slot's pool rows
// back and blanked its reference and interval tables before.
__global__ __launch_bounds__(256) void mt_ckpt_unpack_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                             const uint64_t* __restrict__ off,
                                                             const uint8_t* __restrict__ in) {
    const uint32_t w = blockIdx.x;
    if (w >= n) return;
    const uint32_t d = ids[w];
    const uint32_t tid = blockIdx.y * kCkThreads + threadIdx.x, nth = gridDim.y * kCkThreads;
    const uint8_t* __restrict__ doc = in + off[w];
    const mt_ckpt_dochdr h = *reinterpret_cast<const mt_ckpt_dochdr*>(doc);
    const size_t so = (size_t)d * g.segcap;
    const uint32_t ns = mt_ckpt_nseg(h);
    mt_ckpt_walk(h, [&](int id, uint64_t o, uint64_t b) {
        if (b == 0) return;
        const uint8_t* __restrict__ src = doc + o;
        if (id == CK_OVX0 || id == CK_OVX1) {
            uint4* __restrict__ d4 = reinterpret_cast<uint4*>(g.ovx + MT_OVX_WORDS * so) + (id == CK_OVX1 ? 2 : 0);
            const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(src);
            for (uint64_t v = tid; v < 2ull * ns; v += nth) d4[(v >> 1) * 4 + (v & 1)] = s4[v];
        } else if (uint8_t* dst = ck_engine_ptr(g, d, 0u, id)) {
            ck_copy(dst, src, b, tid, nth);
        }
    });
    if (tid == 0) {
        // the scalars as the blob holds them (text_half 0: the text went into the first half), copied from
        // the blob and not from `h`: a struct store from the by-value copy makes the compiler keep it in LDS
        static_assert(sizeof(mt_doc_scalars) % 16 == 0, "mt_doc_scalars in 16-byte vectors");
        for (uint32_t q = 0; q < sizeof(mt_doc_scalars) / 16; q++)
            reinterpret_cast<uint4*>(g.sc + d)[q] = reinterpret_cast<const uint4*>(doc)[q];
        // An editing client's mt_loc comes with its other sections (mt_ckpt_unpack_loc_kernel, CK_LOC): from
        // the blob's bytes like the scalars, for the same reason.  Any other document is an observer, as
        // mt_init_kernel leaves it.
        if (!(h.flags & MT_CKF_LOC)) {
            g.loc[d].own = -1;
            g.loc[d].glo = g.loc[d].ghi = g.loc[d].stamp = g.loc[d].lseq = g.loc[d].rgn = g.loc[d].rgpn = 0;
        }
        if (g.evn) g.evn[d] = 0;  // events not drained are not part of a checkpoint
        if (g.refs) {
            g.refcur[d] = 0;
            g.refn[d] = 0;
            g.refq[d] = 0;
            g.refdrop[d] = 0;
        }
        if (g.ivs) g.ivn[d] = 0;
    }
}

// The editing sections of the documents that carry MT_CKF_LOC, same grid as the kernels above (a workgroup
// of any other document returns at once).  Pack: the padding was zeroed by mt_ckpt_pack_kernel.  Unpack:
// the host gave the slot one row of each pool its blob's flags name before the launch (locbig / locgx /
// locwx: read here, never written); a section is at most mt_ckpt_nloc entries, the slots of the row it
// lands in, and one whose row is missing is skipped.
__global__ __launch_bounds__(256) void mt_ckpt_pack_loc_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                               const mt_ckpt_dochdr* __restrict__ hdr,
                                                               const uint64_t* __restrict__ off, uint8_t* __restrict__ out) {
    const uint32_t w = blockIdx.x;
    if (w >= n || !(hdr[w].flags & MT_CKF_LOC)) return;
    const uint32_t d = ids[w];
    const uint32_t tid = blockIdx.y * kCkThreads + threadIdx.x, nth = gridDim.y * kCkThreads;
    const mt_ckpt_dochdr h = hdr[w];
    uint8_t* __restrict__ doc = out + off[w];
    const CkRows rows = ck_rows(g, d, h.flags);
    mt_ckpt_walk(h, [&](int id, uint64_t o, uint64_t b) {
        if (id < CK_LOC || id > CK_RGP || b == 0) return;
        if (uint8_t* src = ck_loc_ptr(g, d, id, h.flags, rows)) ck_copy(doc + o, src, b, tid, nth);
    });
}
__global__ __launch_bounds__(256) void mt_ckpt_unpack_loc_kernel(mt_gstate g, const uint32_t* __restrict__ ids, uint32_t n,
                                                                 const uint64_t* __restrict__ off,
                                                                 const uint8_t* __restrict__ in) {
    const uint32_t w = blockIdx.x;
    if (w >= n) return;
    const uint8_t* __restrict__ doc = in + off[w];
    const mt_ckpt_dochdr h = *reinterpret_cast<const mt_ckpt_dochdr*>(doc);
    if (!(h.flags & MT_CKF_LOC)) return;
    const uint32_t d = ids[w];
    const uint32_t tid = blockIdx.y * kCkThreads + threadIdx.x, nth = gridDim.y * kCkThreads;
    const CkRows rows = ck_rows(g, d, h.flags);
    mt_ckpt_walk(h, [&](int id, uint64_t o, uint64_t b) {
        if (id < CK_LOC || id > CK_RGP || b == 0) return;
        if (uint8_t* dst = ck_loc_ptr(g, d, id, h.flags, rows)) ck_copy(dst, doc + o, b, tid, nth);
    });
}

extern "C" hipError_t mt_launch_ckpt_size(const mt_gstate* g, const uint32_t* ids, uint32_t n, mt_ckpt_dochdr* hdr,
                                          hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_ckpt_size_kernel, dim3(n), dim3(64), 0, st, *g, ids, n, hdr);
    return hipGetLastError();
}
extern "C" hipError_t mt_launch_ckpt_pack(const mt_gstate* g, const uint32_t* ids, uint32_t n, const mt_ckpt_dochdr* hdr,
                                          const uint64_t* off, uint8_t* out, uint32_t parts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_ckpt_pack_kernel, dim3(n, parts ? parts : 1), dim3(kCkThreads), 0, st, *g, ids, n, hdr, off, out);
    return hipGetLastError();
}
extern "C" hipError_t mt_launch_ckpt_unpack(const mt_gstate* g, const uint32_t* ids, uint32_t n, const uint64_t* off,
                                            const uint8_t* in, uint32_t parts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_ckpt_unpack_kernel, dim3(n, parts ? parts : 1), dim3(kCkThreads), 0, st, *g, ids, n, off, in);
    return hipGetLastError();
}
extern "C" hipError_t mt_launch_ckpt_pack_loc(const mt_gstate* g, const uint32_t* ids, uint32_t n, const mt_ckpt_dochdr* hdr,
                                              const uint64_t* off, uint8_t* out, uint32_t parts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_ckpt_pack_loc_kernel, dim3(n, parts ? parts : 1), dim3(kCkThreads), 0, st, *g, ids, n, hdr, off, out);
    return hipGetLastError();
}
extern "C" hipError_t mt_launch_ckpt_unpack_loc(const mt_gstate* g, const uint32_t* ids, uint32_t n, const uint64_t* off,
                                                const uint8_t* in, uint32_t parts, hipStream_t st) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(mt_ckpt_unpack_loc_kernel, dim3(n, parts ? parts : 1), dim3(kCkThreads), 0, st, *g, ids, n, off, in);
    return hipGetLastError();
}
