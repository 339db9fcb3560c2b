// mt_ckpt.h -- document checkpoints: the blob format (version 1), its host writer and its host
// checker, and what the kernels of mt_ckpt.hip share with them (DESIGN.md "Checkpoints").
//
// A blob:
//   mt_ckpt_header              32 bytes: magic, version, documents, total bytes, digest
//   mt_ckpt_dirent[n_docs]      {offset, bytes} per document, ascending, back to back
//   documents                   each: mt_ckpt_dochdr (128 bytes), then its sections in the order of
//                               mt_ckpt_sec, each on a 16-byte boundary, padded with zero bytes
// Every section's size follows from the document header alone (mt_ckpt_walk): the sizing kernel, the
// pack and unpack kernels, the host writer and the checker all walk the same list.  The digest covers
// every byte after the header.  Nothing in a blob names a slot, a stride, an arena half or a pool row.
//
// This header is plain C++ on both sides: it needs no HIP header, so a host compiler builds it into a
// stand-alone program as it is (tests/test_checkpoint_host.py).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/mtgpu.h"
#include "mt_checksum.h"  // mt_mix64, MT_HD, MT_OVX_WORDS
#include "mt_state.h"

#define MT_CKPT_MAGIC 0x3154504B434C464Dull  // "MFLCKPT1", little endian
#define MT_CKPT_VERSION 1u

struct mt_ckpt_header {  // 32 bytes
    uint64_t magic;
    uint32_t version;
    uint32_t n_docs;
    uint64_t bytes;   // of the whole blob
    uint64_t digest;  // mt_ckpt_digest of blob[32 .. bytes)
};
struct mt_ckpt_dirent {  // 16 bytes
    uint64_t off, bytes;
};

// mt_ckpt_dochdr.flags
#define MT_CKF_LOC 1u  // an editing client's document (mt_loc.own >= 0): the editing sections follow
#define MT_CKF_BIG 2u  // ... its per-segment editing state held 8192 slots (a big-pool row), not 1024
#define MT_CKF_GX 4u   // ... it held a group-pool row (MT_WIDE_GROUPS): gmx and mt_locx follow
#define MT_CKF_WX 8u   // ... it held a wide-pool row: pkw follows
#define MT_CKF_ALL 15u
// a ghost's index in the reference section: this bit | its index in the table's second half
#define MT_CKPT_GHOST 0x80000000u

struct mt_ckpt_dochdr {  // 128 bytes
    mt_doc_scalars sc;   // as stored, with text_half = 0 (a blob names no arena half)
    uint32_t flags;      // MT_CKF_*
    uint32_t n_refs;     // entries of the reference section: the table's live entries and ghosts (= refn)
    uint32_t n_ivs;      // entries of the interval section (= ivn)
    uint32_t refdrop;    // mt_refs_dropped
    uint32_t rgn, rgpn;  // regenerated ops not drained: records, payload bytes (= mt_loc's)
    uint32_t pad[6];
};

enum mt_ckpt_sec {
    CK_SEQ, CK_RSEQ, CK_LEN, CK_TOFF, CK_OVL, CK_PROPS, CK_CLIENT, CK_RCLIENT, CK_FLAGS,  // nseg entries
    CK_CHI, CK_PH, CK_PXL, CK_PXH, CK_OVX0,  // a wide document's (ovx words 0..3 per segment)
    CK_PXX,                                  // ... with MT_WIDE_XKV
    CK_OVX1,                                 // ... with MT_WIDE_XOV (ovx words 4..7)
    CK_SLAB,                                 // label keys declared
    CK_LBCNT, CK_LBSCOUR,                    // nb[0] entries
    CK_IB1, CK_IB2, CK_IB3, CK_IB4, CK_IB5, CK_IB6,  // nb[l] entries, l < nlev
    CK_HSEQ, CK_HSLOT,                       // heap entries 1 .. heap_n
    CK_TEXT,                                 // text_top units (a wide document: 2 bytes each)
    CK_LOC, CK_GM, CK_PK, CK_CT, CK_LSQ,     // MT_CKF_LOC: mt_loc, then mt_ckpt_nloc entries each
    CK_GMX, CK_LOCX,                         // MT_CKF_GX
    CK_PKW,                                  // MT_CKF_WX
    CK_RG, CK_RGP,                           // rgn records, rgpn bytes
    CK_REFIDX, CK_REFS,                      // n_refs: index (ascending; ghosts after references), mt_ref
    CK_IVIDX, CK_IVS,                        // n_ivs: index (ascending), mt_interval
    CK_NSEC
};

MT_HD static inline uint32_t mt_ckpt_nseg(const mt_ckpt_dochdr& h) { return h.sc.nseg > 0 ? (uint32_t)h.sc.nseg : 0u; }
// per-segment entries of an editing document's state: what its row holds
MT_HD static inline uint32_t mt_ckpt_nloc(const mt_ckpt_dochdr& h) {
    const uint32_t n = mt_ckpt_nseg(h), cap = (h.flags & MT_CKF_BIG) ? MT_LOC_BIGCAP : MT_LOC_CAP;
    return n < cap ? n : cap;
}
MT_HD static inline uint64_t mt_ckpt_align(uint64_t b) { return (b + 15) & ~(uint64_t)15; }

// Calls f(section, offset in the document, bytes) for every section of a document, in order, absent
// sections with 0 bytes; returns the document's bytes.  All arithmetic in 64 bits: the counts are
// 32-bit and an element is at most 4 KiB.
template <class F>
MT_HD static inline uint64_t mt_ckpt_walk(const mt_ckpt_dochdr& h, F&& f) {
    uint64_t off = sizeof(mt_ckpt_dochdr);
#define MT_CK_SEC(id, on, count, esize)                                  \
    {                                                                    \
        const uint64_t b_ = (on) ? (uint64_t)(count) * (esize) : 0ull;   \
        f(id, off, b_);                                                  \
        off += mt_ckpt_align(b_);                                        \
    }
    const mt_doc_scalars& sc = h.sc;
    const uint64_t ns = mt_ckpt_nseg(h), nl = mt_ckpt_nloc(h);
    const bool wide = (sc.wide & MT_WIDE_DOC) != 0, loc = (h.flags & MT_CKF_LOC) != 0;
    const uint64_t hn = sc.heap_n > 0 ? (uint64_t)sc.heap_n : 0ull;
    MT_CK_SEC(CK_SEQ, true, ns, 4)
    MT_CK_SEC(CK_RSEQ, true, ns, 4)
    MT_CK_SEC(CK_LEN, true, ns, 4)
    MT_CK_SEC(CK_TOFF, true, ns, 4)
    MT_CK_SEC(CK_OVL, true, ns, 8)
    MT_CK_SEC(CK_PROPS, true, ns, 8)
    MT_CK_SEC(CK_CLIENT, true, ns, 1)
    MT_CK_SEC(CK_RCLIENT, true, ns, 1)
    MT_CK_SEC(CK_FLAGS, true, ns, 1)
    MT_CK_SEC(CK_CHI, wide, ns, 2)
    MT_CK_SEC(CK_PH, wide, ns, 8)
    MT_CK_SEC(CK_PXL, wide, ns, 8)
    MT_CK_SEC(CK_PXH, wide, ns, 8)
    MT_CK_SEC(CK_OVX0, wide, ns, 32)
    MT_CK_SEC(CK_PXX, wide && (sc.wide & MT_WIDE_XKV), ns, 32)
    MT_CK_SEC(CK_OVX1, wide && (sc.wide & MT_WIDE_XOV), ns, 32)
    MT_CK_SEC(CK_SLAB, sc.label_keys != MT_NO_LABEL_KEYS, ns, 4)
    MT_CK_SEC(CK_LBCNT, true, sc.nb[0] > 0 ? sc.nb[0] : 0, 1)
    MT_CK_SEC(CK_LBSCOUR, true, sc.nb[0] > 0 ? sc.nb[0] : 0, 1)
    MT_CK_SEC(CK_IB1, sc.nlev > 1 && sc.nb[1] > 0, sc.nb[1], 1)
    MT_CK_SEC(CK_IB2, sc.nlev > 2 && sc.nb[2] > 0, sc.nb[2], 1)
    MT_CK_SEC(CK_IB3, sc.nlev > 3 && sc.nb[3] > 0, sc.nb[3], 1)
    MT_CK_SEC(CK_IB4, sc.nlev > 4 && sc.nb[4] > 0, sc.nb[4], 1)
    MT_CK_SEC(CK_IB5, sc.nlev > 5 && sc.nb[5] > 0, sc.nb[5], 1)
    MT_CK_SEC(CK_IB6, sc.nlev > 6 && sc.nb[6] > 0, sc.nb[6], 1)
    MT_CK_SEC(CK_HSEQ, true, hn, 4)
    MT_CK_SEC(CK_HSLOT, true, hn, 2)
    MT_CK_SEC(CK_TEXT, true, sc.text_top, wide ? 2 : 1)
    MT_CK_SEC(CK_LOC, loc, 1, sizeof(mt_loc))
    MT_CK_SEC(CK_GM, loc, nl, 8)
    MT_CK_SEC(CK_PK, loc, nl, 8)
    MT_CK_SEC(CK_CT, loc, nl, 4)
    MT_CK_SEC(CK_LSQ, loc, nl, 8)
    MT_CK_SEC(CK_GMX, loc && (h.flags & MT_CKF_GX), nl, 8 * MT_LOC_GW)
    MT_CK_SEC(CK_LOCX, loc && (h.flags & MT_CKF_GX), 1, sizeof(mt_locx))
    MT_CK_SEC(CK_PKW, loc && (h.flags & MT_CKF_WX), nl, 8 * MT_PKW_WORDS)
    MT_CK_SEC(CK_RG, loc, h.rgn, sizeof(mt_op_rec))
    MT_CK_SEC(CK_RGP, loc, h.rgpn, 1)
    MT_CK_SEC(CK_REFIDX, true, h.n_refs, 4)
    MT_CK_SEC(CK_REFS, true, h.n_refs, sizeof(mt_ref))
    MT_CK_SEC(CK_IVIDX, true, h.n_ivs, 4)
    MT_CK_SEC(CK_IVS, true, h.n_ivs, sizeof(mt_interval))
#undef MT_CK_SEC
    return off;
}
MT_HD static inline uint64_t mt_ckpt_doc_bytes(const mt_ckpt_dochdr& h) {
    return mt_ckpt_walk(h, [](int, uint64_t, uint64_t) {});
}

// ---- host side -------------------------------------------------------------------------------------
#include <algorithm>
#include <thread>
#include <vector>

static_assert(sizeof(mt_ckpt_header) == 32 && sizeof(mt_ckpt_dirent) == 16 && sizeof(mt_ckpt_dochdr) == 128 &&
                  sizeof(mt_doc_scalars) == 80 && sizeof(mt_ref) == 16 && sizeof(mt_interval) == 16 &&
                  sizeof(mt_loc) == 540 && sizeof(mt_locx) == 4096 && sizeof(mt_op_rec) == 32,
              "the records of checkpoint format 1");

// The digest of p[0 .. bytes) (bytes a multiple of 8): every 64-bit word mixed with its index, the
// results xor-ed -- any order, so a large blob is hashed on all host cores (mt_mix64: mt_synth.h).
static inline uint64_t mt_ckpt_digest_range(const uint8_t* p, uint64_t w0, uint64_t w1) {
    uint64_t x = 0;
    for (uint64_t i = w0; i < w1; i++) {
        uint64_t w;
        memcpy(&w, p + 8 * i, 8);
        x ^= mt_mix64(w ^ mt_mix64(i));
    }
    return x;
}
static inline unsigned mt_ckpt_threads(uint64_t bytes) {
    if (bytes < (16ull << 20)) return 1;
    return std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u);
}
static inline uint64_t mt_ckpt_digest(const uint8_t* p, uint64_t bytes) {
    const uint64_t nw = bytes / 8;
    const unsigned nt = mt_ckpt_threads(bytes);
    uint64_t x = 0;
    if (nt == 1) {
        x = mt_ckpt_digest_range(p, 0, nw);
    } else {
        std::vector<uint64_t> part(nt, 0);
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++)
            th.emplace_back([&, t] { part[t] = mt_ckpt_digest_range(p, nw * t / nt, nw * (t + 1) / nt); });
        for (auto& q : th) q.join();
        for (uint64_t v : part) x ^= v;
    }
    return mt_mix64(x ^ nw);
}

// bytes of the header and directory of a blob of n documents
static inline uint64_t mt_ckpt_front(uint64_t n) { return sizeof(mt_ckpt_header) + n * sizeof(mt_ckpt_dirent); }
// Writes the header and the directory of a blob whose documents (doc_bytes[i] each, already in
// place back to back from mt_ckpt_front(n)) are complete, and seals it with the digest.
static inline void mt_ckpt_seal(uint8_t* blob, uint64_t bytes) {
    mt_ckpt_header h;
    memcpy(&h, blob, sizeof h);
    h.digest = mt_ckpt_digest(blob + sizeof h, bytes - sizeof h);
    memcpy(blob, &h, sizeof h);
}
static inline void mt_ckpt_write_front(uint8_t* blob, uint32_t n, const uint64_t* doc_bytes) {
    uint64_t off = mt_ckpt_front(n);
    for (uint32_t i = 0; i < n; i++) {
        const mt_ckpt_dirent de{off, doc_bytes[i]};
        memcpy(blob + sizeof(mt_ckpt_header) + (uint64_t)i * sizeof de, &de, sizeof de);
        off += doc_bytes[i];
    }
    const mt_ckpt_header h{MT_CKPT_MAGIC, MT_CKPT_VERSION, n, off, 0};
    memcpy(blob, &h, sizeof h);
    mt_ckpt_seal(blob, off);
}

// The writer: one document from its header and the bytes of its sections (sec[id]: at least the
// section's size, or empty for zeros), appended to `out`.
struct mt_ckpt_hostdoc {
    mt_ckpt_dochdr h{};
    std::vector<uint8_t> sec[CK_NSEC];
    template <class T>
    void put(int id, const std::vector<T>& v) {
        sec[id].resize(v.size() * sizeof(T));
        if (!v.empty()) memcpy(sec[id].data(), v.data(), sec[id].size());
    }
};
static inline void mt_ckpt_write_doc(const mt_ckpt_hostdoc& d, std::vector<uint8_t>& out) {
    const size_t base = out.size();
    out.resize(base + mt_ckpt_doc_bytes(d.h), 0);
    memcpy(out.data() + base, &d.h, sizeof d.h);
    mt_ckpt_walk(d.h, [&](int id, uint64_t off, uint64_t b) {
        const uint64_t have = std::min<uint64_t>(b, d.sec[id].size());
        if (have) memcpy(out.data() + base + off, d.sec[id].data(), have);
    });
}
// a blob of documents written by mt_ckpt_write_doc
static inline std::vector<uint8_t> mt_ckpt_write_blob(const std::vector<std::vector<uint8_t>>& docs) {
    std::vector<uint64_t> sz;
    uint64_t total = mt_ckpt_front(docs.size());
    for (auto& d : docs) {
        sz.push_back(d.size());
        total += d.size();
    }
    std::vector<uint8_t> blob(total, 0);
    uint64_t off = mt_ckpt_front(docs.size());
    for (auto& d : docs) {
        if (!d.empty()) memcpy(blob.data() + off, d.data(), d.size());
        off += d.size();
    }
    mt_ckpt_write_front(blob.data(), (uint32_t)docs.size(), sz.data());
    return blob;
}

// ---- the checker -------------------------------------------------------------------------------------
// Header and directory: in bounds, aligned, documents back to back in order.  (No digest.)
static inline uint32_t mt_ckpt_check_front(const uint8_t* blob, uint64_t bytes, mt_ckpt_header* out) {
    mt_ckpt_header h;
    if (!blob || bytes < sizeof h) return MT_CKW_TRUNCATED;
    memcpy(&h, blob, sizeof h);
    if (h.magic != MT_CKPT_MAGIC) return MT_CKW_MAGIC;
    if (h.version != MT_CKPT_VERSION) return MT_CKW_VERSION;
    if (h.bytes > bytes) return MT_CKW_TRUNCATED;
    if (h.bytes != bytes || (bytes & 15)) return MT_CKW_DIRECTORY;
    const uint64_t front = mt_ckpt_front(h.n_docs);
    if (front > bytes) return MT_CKW_TRUNCATED;
    uint64_t off = front;
    for (uint32_t i = 0; i < h.n_docs; i++) {
        mt_ckpt_dirent de;
        memcpy(&de, blob + sizeof h + (uint64_t)i * sizeof de, sizeof de);
        if (de.off != off || de.bytes < sizeof(mt_ckpt_dochdr) || (de.bytes & 15) || de.bytes > bytes - off)
            return MT_CKW_DIRECTORY;
        off += de.bytes;
    }
    if (off != bytes) return MT_CKW_DIRECTORY;
    if (out) *out = h;
    return MT_CKW_OK;
}
static inline mt_ckpt_dirent mt_ckpt_dir(const uint8_t* blob, uint32_t i) {
    mt_ckpt_dirent de;
    memcpy(&de, blob + sizeof(mt_ckpt_header) + (uint64_t)i * sizeof de, sizeof de);
    return de;
}

// the largest counts any engine holds (mt_engine_impl.h kMaxSegCap and its block capacities)
#define MT_CKPT_MAX_SEG 65472
#define MT_CKPT_MAX_HEAP (1 << 20)

// One document of `bytes` bytes at p (16-byte aligned in its blob): every invariant a kernel trusts.
static inline uint32_t mt_ckpt_check_doc(const uint8_t* p, uint64_t bytes) {
    mt_ckpt_dochdr h;
    if (bytes < sizeof h) return MT_CKW_SIZE;
    memcpy(&h, p, sizeof h);
    const mt_doc_scalars& sc = h.sc;
    // scalars: everything the section sizes are computed from, first
    if (sc.nseg < 0 || sc.nseg > MT_CKPT_MAX_SEG || sc.nlev < 1 || sc.nlev > MT_MAXLEV) return MT_CKW_SCALARS;
    for (int l = 0; l < sc.nlev; l++)
        if (sc.nb[l] < 1 || sc.nb[l] > (l == 0 ? MT_CKPT_MAX_SEG / 2 : MT_CKPT_MAX_SEG / 8 + 8)) return MT_CKW_SCALARS;
    if (sc.nb[sc.nlev - 1] != 1) return MT_CKW_SCALARS;
    const bool wide = (sc.wide & MT_WIDE_DOC) != 0;
    if (sc.heap_n < 0 || sc.heap_n > MT_CKPT_MAX_HEAP || sc.min_seq > sc.cur_seq || sc.text_half != 0 ||
        (uint64_t)sc.text_top * (wide ? 2u : 1u) > MT_MAX_TEXTCAP || sc.n_empty > (uint32_t)sc.nb[0] || sc.err < 0 ||
        sc.err > MT_DERR_EVENTS || sc.win_op < -2)
        return MT_CKW_SCALARS;
    if ((h.flags & ~MT_CKF_ALL) || ((h.flags & (MT_CKF_BIG | MT_CKF_GX | MT_CKF_WX)) && !(h.flags & MT_CKF_LOC)))
        return MT_CKW_SCALARS;
    for (uint32_t k : h.pad)
        if (k) return MT_CKW_SCALARS;
    // the rows a document held agree with its form: a group row with MT_WIDE_GROUPS (a halted document may
    // have been refused its row), a wide row with a wide document, declared label keys with the LDS engine
    if (((h.flags & MT_CKF_GX) && !(sc.wide & MT_WIDE_GROUPS)) ||
        ((h.flags & MT_CKF_LOC) && (sc.wide & MT_WIDE_GROUPS) && !(h.flags & MT_CKF_GX) && !sc.err) ||
        ((h.flags & MT_CKF_WX) && !wide) || (sc.label_keys != MT_NO_LABEL_KEYS && !(sc.wide & MT_WIDE_LDS)))
        return MT_CKW_SCALARS;
    if (sc.label_keys != MT_NO_LABEL_KEYS) {
        if (sc.label_keys >> 16) return MT_CKW_IDS;
        for (int s = 0; s < 16; s += 8) {
            const uint32_t k = (sc.label_keys >> s) & 0xFFu;
            if (k != 0xFFu && k >= MT_MAX_KEYS_WIDE) return MT_CKW_IDS;
        }
    }
    if (h.n_refs > 2 * MT_REFS_MAX) return MT_CKW_REFS;
    if (h.n_ivs > MT_INTERVALS_MAX) return MT_CKW_INTERVALS;
    if (h.rgn > MT_RG_RECS || h.rgpn > MT_RG_BYTES || (!(h.flags & MT_CKF_LOC) && (h.rgn || h.rgpn))) return MT_CKW_PENDING;
    const uint8_t* s[CK_NSEC];
    const uint64_t need = mt_ckpt_walk(h, [&](int id, uint64_t off, uint64_t b) {
        s[id] = p + off;  // (read only after the size check below)
    });
    if (need != bytes) return MT_CKW_SIZE;
    auto u8 = [&](int id, uint64_t i) { return s[id][i]; };
    auto u16 = [&](int id, uint64_t i) { uint16_t v; memcpy(&v, s[id] + 2 * i, 2); return v; };
    auto u32 = [&](int id, uint64_t i) { uint32_t v; memcpy(&v, s[id] + 4 * i, 4); return v; };
    const uint32_t ns = (uint32_t)sc.nseg;
    // the padding between sections is zero (so equal states give equal bytes)
    {
        bool dirty = false;
        mt_ckpt_walk(h, [&](int, uint64_t off, uint64_t b) {
            for (uint64_t q = off + b; q < off + mt_ckpt_align(b); q++) dirty |= p[q] != 0;
        });
        if (dirty) return MT_CKW_SIZE;
    }
    // blocks
    {
        uint64_t sum = 0, empty = 0;
        for (int32_t b = 0; b < sc.nb[0]; b++) {
            const uint32_t c = u8(CK_LBCNT, b);
            if (c > 8 || u8(CK_LBSCOUR, b) > MT_SC_FALSE) return MT_CKW_BLOCKS;
            sum += c;
            empty += c == 0;
        }
        // (a document halted over a capacity stopped mid-op, and nothing applies to it again: its counts
        // stay within their bounds but need not add up)
        if (!sc.err && (sum != ns || empty != sc.n_empty)) return MT_CKW_BLOCKS;
        for (int l = 1; l < sc.nlev; l++) {
            sum = 0;
            for (int32_t b = 0; b < sc.nb[l]; b++) {
                const uint32_t c = u8(CK_IB1 + l - 1, b);
                if (c > 8) return MT_CKW_BLOCKS;
                sum += c;
            }
            if (!sc.err && sum != (uint64_t)sc.nb[l - 1]) return MT_CKW_BLOCKS;
        }
    }
    // segments: text ranges and client ids
    for (uint32_t i = 0; i < ns; i++) {
        if ((uint64_t)u32(CK_TOFF, i) + u32(CK_LEN, i) > sc.text_top) return MT_CKW_TEXT;
        const uint32_t fl = u8(CK_FLAGS, i);
        uint32_t c = u8(CK_CLIENT, i), rc = u8(CK_RCLIENT, i);
        if (wide) {
            const uint32_t hi = u16(CK_CHI, i);
            c |= (hi & 0xFFu) << 8;
            rc |= (hi >> 8) << 8;
        }
        const uint32_t lim = wide ? MT_MAX_CLIENTS_WIDE : MT_MAX_CLIENTS;
        if (c >= lim && c != MT_CLIENT_NONCOLLAB) return MT_CKW_IDS;
        if ((fl & MT_SF_REMOVED) && rc >= lim) return MT_CKW_IDS;
    }
    // heap
    for (int32_t i = 0; i < sc.heap_n; i++) {
        const uint32_t v = u16(CK_HSLOT, i);
        if (v >= ns && v != MT_DEAD_SLOT) return MT_CKW_HEAP;
    }
    // an editing client's pending state
    if (h.flags & MT_CKF_LOC) {
        mt_loc lc;
        memcpy(&lc, s[CK_LOC], sizeof lc);
        const uint32_t cap = (h.flags & MT_CKF_GX) ? MT_LOC_GROUPS_WIDE : 64u;  // (what its sections hold)
        if (lc.own < 0 || (uint32_t)lc.own >= (wide ? MT_MAX_CLIENTS_WIDE : MT_MAX_CLIENTS)) return MT_CKW_IDS;
        if (lc.glo > lc.ghi || lc.ghi - lc.glo > cap || lc.rgn != h.rgn || lc.rgpn != h.rgpn) return MT_CKW_PENDING;
        if (ns > mt_ckpt_nloc(h) && !sc.err) return MT_CKW_PENDING;  // (more segments than its row holds)
        for (uint32_t i = 0; i < h.rgn; i++) {
            mt_op_rec r;
            memcpy(&r, s[CK_RG] + (uint64_t)i * sizeof r, sizeof r);
            if ((uint64_t)r.payload_off + r.payload_len > h.rgpn) return MT_CKW_PENDING;
        }
    }
    // references: indices ascending (references, then ghosts), settled, ordinals inside the document
    for (uint32_t i = 0; i < h.n_refs; i++) {
        const uint32_t ix = u32(CK_REFIDX, i);
        if ((ix & ~MT_CKPT_GHOST) >= MT_REFS_MAX || (i && ix <= u32(CK_REFIDX, i - 1))) return MT_CKW_REFS;
        mt_ref r;
        memcpy(&r, s[CK_REFS] + (uint64_t)i * sizeof r, sizeof r);
        const bool ghost = (ix & MT_CKPT_GHOST) != 0;
        if (r.ord < -1 || r.ord >= (int32_t)ns) return MT_CKW_REFS;
        if ((r.flags & (MT_RF_PENDING | MT_RF_ZOMBIE)) || ghost != ((r.flags & MT_RF_GHOST) != 0) ||
            ghost == ((r.flags & MT_RF_LIVE) != 0))
            return MT_CKW_REFS;
    }
    // intervals: indices ascending, endpoints stored references
    for (uint32_t i = 0; i < h.n_ivs; i++) {
        const uint32_t ix = u32(CK_IVIDX, i);
        if (ix >= MT_INTERVALS_MAX || (i && ix <= u32(CK_IVIDX, i - 1))) return MT_CKW_INTERVALS;
        mt_interval v;
        memcpy(&v, s[CK_IVS] + (uint64_t)i * sizeof v, sizeof v);
        if (!v.live) return MT_CKW_INTERVALS;
        for (uint32_t e : {v.start, v.end}) {
            bool found = false;
            for (uint32_t lo = 0, hi = h.n_refs; lo < hi;) {  // (ascending: binary search)
                const uint32_t mid = (lo + hi) / 2, x = u32(CK_REFIDX, mid);
                if (x == e) {
                    found = true;
                    break;
                }
                if (x < e) lo = mid + 1;
                else hi = mid;
            }
            if (!found || (e & MT_CKPT_GHOST)) return MT_CKW_INTERVALS;
        }
    }
    return MT_CKW_OK;
}

// The whole blob.  0: good; else the reason, with *bad the document (0xFFFFFFFF: the header).
static inline uint32_t mt_ckpt_check(const uint8_t* blob, uint64_t bytes, uint32_t* n_docs, uint32_t* bad) {
    mt_ckpt_header h;
    if (bad) *bad = 0xFFFFFFFFu;
    if (n_docs) *n_docs = 0;
    uint32_t why = mt_ckpt_check_front(blob, bytes, &h);
    if (why) return why;
    if (mt_ckpt_digest(blob + sizeof h, bytes - sizeof h) != h.digest) return MT_CKW_DIGEST;
    if (n_docs) *n_docs = h.n_docs;
    const unsigned nt = h.n_docs < 64 ? 1u : mt_ckpt_threads(bytes);
    std::vector<uint32_t> first(nt, 0xFFFFFFFFu), fwhy(nt, 0);
    auto range = [&](unsigned t) {
        for (uint64_t i = (uint64_t)h.n_docs * t / nt, hi = (uint64_t)h.n_docs * (t + 1) / nt; i < hi; i++) {
            const mt_ckpt_dirent de = mt_ckpt_dir(blob, (uint32_t)i);
            const uint32_t w = mt_ckpt_check_doc(blob + de.off, de.bytes);
            if (w) {
                first[t] = (uint32_t)i;
                fwhy[t] = w;
                return;
            }
        }
    };
    if (nt == 1) {
        range(0);
    } else {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < nt; t++) th.emplace_back(range, t);
        for (auto& q : th) q.join();
    }
    for (unsigned t = 0; t < nt; t++)
        if (fwhy[t]) {  // (the lowest failing document: the ranges ascend)
            if (bad) *bad = first[t];
            return fwhy[t];
        }
    return MT_CKW_OK;
}
