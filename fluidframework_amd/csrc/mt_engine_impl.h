// mt_engine_impl.h -- what the host files of libmtgpu.so share: the engine and batch objects behind
// the opaque handles of include/mtgpu.h, the constants their layout depends on, and the HIP error /
// allocation helpers.  mt_engine.cpp (lifecycle, apply scheduling, ticks, synth), mt_queries.cpp (the
// query entry points) and mt_readout.cpp (the canonical readout) include it; nothing else does.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mtgpu.h"
#include "mt_launch.h"
#include "mt_state.h"

// register engine <= 1024, LDS engine 2048, the LDS engine's HBM-workspace form above (only the
// classes with CAP <= the engine's seg_capacity are used: mt_engine::n_classes); the classes' tables
// (kClasses, kClassParams, ...) are the apply scheduler's, in mt_engine.cpp
constexpr int kNumClasses = 21;
constexpr int kLdsClasses = 16;  // classes an LDS-resident kernel serves (the generator's)
constexpr int kFirstLds = 15;    // index of the 2048 class: the first the register engine does not serve
constexpr int kMaxSegCap = 65472;  // (the LDS engine's slot indices are u16: Lds::order / hslot)
// bins of a tick (mt_bin_kernel): the classes, the editing documents, and the wide documents of the
// classes from 2048 up (the LDS engine's wide form, include/mtgpu.h "limits")
// the wide form serves the classes from 256 segments on: up to 512 staged in LDS, above in the HBM
// workspace (mt_launch_apply_wide)
constexpr int kFirstWide = 2;
constexpr int kWideClasses = kNumClasses - kFirstWide;
// ... and, after those, per register class: the documents that need the LDS engine there (declared
// label keys), run by the LDS engine at that class's capacity, then the documents with client ids
// above 32, run by the register engine's C64 form (mt_bin_kernel)
// (then the editing documents that fit 256 / 512 slots: the editing form at that size; then those
// above MT_LOC_CAP = 1024: its HBM-workspace form at 2048 / 4096; then those past 64 pending edits
// (MT_WIDE_GROUPS): the HBM-workspace form with 4 group-mask words per slot at 1024 / 4096; then
// both forms at 8192; then the wide editing forms (include/mtgpu.h "limits": an editing document past the
// narrow limits) at 1024 / 4096 / 8192 slots, with one group-mask word per slot and then with MT_LOC_GW)
constexpr int kLocForms = 14;
constexpr int kBuckets = kNumClasses + 1 + kWideClasses + 2 * kFirstLds + kLocForms;
// binning's counters: one per bucket, then per wide bucket the documents that stage the wide form's
// extension (mt_state.h MT_WIDE_XK / MT_WIDE_XO) -- their launch takes an HBM region for it
constexpr int kCounts = kBuckets + kWideClasses;
// per-class statistics: the classes, the editing bucket, the LDS engine inside each register class,
// the register engine's C64 form per class, the other editing forms
constexpr int kStatClasses = kNumClasses + 1 + 2 * kFirstLds + kLocForms + kWideClasses;
constexpr int kStatWide = kNumClasses + 1 + 2 * kFirstLds + kLocForms;  // the wide form's entries

struct mt_batch {
    mt_op_rec* ops = nullptr;
    uint8_t* payload = nullptr;
    uint32_t* row_ptr = nullptr;
    uint64_t n_ops = 0, payload_bytes = 0;
    uint32_t n_docs = 0;
    uint32_t max_ops_per_doc = 0;
    bool wide = false;  // some record needs the wide form (its documents' wide state is allocated first)
};

struct mt_engine {
    mt_cfg cfg{};
    hipStream_t stream = nullptr;
    mt_gstate g{};
    uint32_t n_docs = 0;
    std::vector<void*> allocs;
    int32_t* d_classes = nullptr;
    uint32_t* d_counts = nullptr;
    uint32_t* d_ids = nullptr;
    uint32_t* h_counts = nullptr;  // pinned
    unsigned long long* d_acc = nullptr;
    std::vector<hipEvent_t> kev;   // per apply launch: start/stop pairs
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    float last_ms = 0.f, last_wall_ms = 0.f;
    // per capacity class, plus one entry for the editing documents' bucket (index kNumClasses)
    float cls_ms[kStatClasses] = {0};
    uint32_t cls_launches[kStatClasses] = {0};
    uint64_t cls_bytes[kStatClasses] = {0};
    std::vector<int> kev_cls;
    uint32_t last_launches = 0;
    uint64_t last_bytes = 0;
    // register-resident engine (mt_apply_reg.hip) for classes up to kRegMaxCap segments; the
    // LDS engine (mt_apply.hip) above that, or everywhere with MTGPU_ENGINE=lds
    bool use_reg = true;
    bool reg_default = true;       // use_reg when not recording delta events (mt_events_enable)
    int n_classes = kLdsClasses;   // classes with CAP <= seg_capacity
    int first_lds = kFirstLds;     // first class not served by the register engine
    uint8_t* ws = nullptr;         // HBM workspace of the classes above 2048 segments
    size_t ws_bytes = 0;
    // the capacity classes of one tick touch disjoint documents: each runs on its own stream
    // (fork/join around the tick) so the small classes and every class's tail overlap;
    // MTGPU_SERIAL=1 keeps them on the engine stream, one after another
    bool concurrent = true;
    bool desc_order = true;  // class kernels launched largest capacity first (see apply_launches)
    hipStream_t side[kNumClasses] = {};
    hipEvent_t fork_ev = nullptr, join_ev[kNumClasses] = {};
    uint64_t gen = 0;  // bumped by every call that can change document state (snap_cache's key)
    std::vector<uint16_t> lkeys;  // per document: its declared label keys (mt_set_label_keys), host copy
    // the editing documents' pool rows (mt_state.h locbig / locgx): host copies, rows in use, rows held
    std::vector<uint32_t> h_locbig, h_locgx, h_locwx, h_bucket;
    uint32_t nbig = 0, bigcap = 0, ngx = 0, gxcap = 0, nwx = 0, wxcap = 0;
    std::vector<uint32_t> free_big, free_gx, free_wx;  // rows given back by reloaded documents, reused first
    // mt_submit_ticks: a ring of device slots; tick k is copied into slot k % kRing on the h2d
    // stream while the ticks before it apply, and the slot is reused once its tick has applied (and
    // its tickets have gone back on the d2h stream)
    struct TickSlot {
        mt_op_rec* ops = nullptr;
        uint8_t* pay = nullptr;
        uint32_t* rp = nullptr;
        mt_raw_msg* msgs = nullptr;
        uint32_t* mrp = nullptr;
        mt_ticket* tk = nullptr;
        uint64_t ops_cap = 0, pay_cap = 0, msg_cap = 0;
        hipEvent_t ready = nullptr, applied = nullptr, drained = nullptr, ticketed = nullptr;
    } ring[6];
    hipStream_t h2d = nullptr, d2h = nullptr;
    uint32_t* d_scan = nullptr;  // the first tick's record check on the device (mt_scan_records_kernel)
    struct {  // mt_get_snapshots: the JSON of the last sizing call
        bool valid = false;
        uint64_t gen = 0;
        uint32_t d0 = 0, n = 0, chunk = 0, n_names = 0;
        const char* const* names = nullptr;
        std::string json;
        std::vector<uint64_t> off;
    } snap_cache;
    struct {  // mt_docs_save: the sizing of the last call (the documents, their headers and offsets on the device)
        bool valid = false;
        uint64_t gen = 0, total = 0, max_doc = 0;
        std::vector<uint32_t> ids;
        void* dev = nullptr;  // one allocation: ids, headers, offsets
        size_t o_hdr = 0, o_off = 0;
        bool unsupported = false;  // a document save refuses (mt_engine.cpp ckpt_supported)
        bool any_loc = false;      // an editing client's document among them (its sections: a launch of their own)
    } ckpt_cache;
    // mt_last_checkpoint_stats: the last pack / unpack launch by HIP events, and the blob bytes it moved
    float ckpt_pack_ms = 0.f, ckpt_unpack_ms = 0.f;
    uint64_t ckpt_pack_bytes = 0, ckpt_unpack_bytes = 0;
};

#define HIP_OK(x)                                                                                            \
    do {                                                                                                     \
        hipError_t e_ = (x);                                                                                 \
        if (e_ != hipSuccess) {                                                                              \
            fprintf(stderr, "libmtgpu: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
            return MT_ERR_HIP;                                                                               \
        }                                                                                                    \
    } while (0)

template <class T>
static mt_status dalloc(mt_engine* e, T** p, size_t count) {
    void* q = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return MT_ERR_NOMEM;
    e->allocs.push_back(q);
    *p = static_cast<T*>(q);
    return MT_OK;
}

// the interval tables (mt_intervals_enable)
static inline void intervals_free(mt_engine* e) {
    if (e->g.ivs) (void)hipFree(e->g.ivs);
    if (e->g.ivn) (void)hipFree(e->g.ivn);
    e->g.ivs = nullptr;
    e->g.ivn = nullptr;
    e->g.ivcap = 0;
}
// the local-reference tables (mt_refs_enable), and the intervals that rest on them
static inline void refs_free(mt_engine* e) {
    intervals_free(e);
    for (void* p : {(void*)e->g.refs, (void*)e->g.refpos, (void*)e->g.refcur, (void*)e->g.refn, (void*)e->g.refq,
                    (void*)e->g.refdrop})
        if (p) (void)hipFree(p);
    e->g.refs = nullptr;
    e->g.refpos = nullptr;
    e->g.refcur = e->g.refn = e->g.refq = e->g.refdrop = nullptr;
    e->g.refcap = 0;
}
// every document's references freed, cursors at the start of the event buffer
static inline hipError_t refs_clear(mt_engine* e) {
    if (!e->g.refs) return hipSuccess;
    const size_t D = e->cfg.max_docs;
    hipError_t r = hipMemsetAsync(e->g.refs, 0, D * 2 * e->g.refcap * sizeof(mt_ref), e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(e->g.refcur, 0, D * sizeof(uint32_t), e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(e->g.refn, 0, D * sizeof(uint32_t), e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(e->g.refq, 0, D * sizeof(uint32_t), e->stream);
    if (r == hipSuccess) r = hipMemsetAsync(e->g.refdrop, 0, D * sizeof(uint32_t), e->stream);
    if (r == hipSuccess && e->g.ivs) r = mt_launch_intervals_free_docs(&e->g, nullptr, e->cfg.max_docs, e->cfg.max_docs, e->stream);
    return r;
}
