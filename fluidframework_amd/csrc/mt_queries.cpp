// mt_queries.cpp -- the query entry points of libmtgpu.so (include/mtgpu.h): tiles, positions, marker
// ids, segment infos and text, the regeneration drain, stacks, events, local references, interval
// collections, text reads, checksums, segment counts and the document error.
//
// A batched query is one round trip on the engine stream (mt_scratch.h): argument check, the
// layout of one scratch block, the chain of copies and launches, return.  Refusals come in this
// order: MT_ERR_ARG (the per-query document check included) before any device work, then
// MT_ERR_NOMEM, then MT_ERR_HIP.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mt_engine_impl.h"
#include "mt_scratch.h"

extern "C" {

mt_status mt_find_tiles(mt_engine* e, const mt_tile_query* q, uint32_t n, mt_tile_result* out) {
    static_assert(sizeof(mt_tile_query) == 48, "mt_tile_query is 48 bytes");
    if (!e || (n && (!q || !out)) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, dr] = s.carve<mt_tile_query, mt_tile_result>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_tiles, &e->g, dq, n, dr, e->stream)
        .d2h(out, dr, n * sizeof *out)
        .sync().status();
}

mt_status mt_resolve_positions(mt_engine* e, const mt_pos_query* q, uint32_t n, mt_pos_result* out) {
    static_assert(sizeof(mt_pos_query) == 16 && sizeof(mt_pos_result) == 16, "mt_pos_query / result are 16 bytes");
    if (!e || (n && (!q || !out)) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    for (uint32_t i = 0; i < n; i++)
        if (q[i].kind > MT_POS_OF_ORDINAL) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, dr] = s.carve<mt_pos_query, mt_pos_result>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_resolve, &e->g, dq, n, e->n_docs, dr, e->stream)
        .d2h(out, dr, n * sizeof *out)
        .sync().status();
}

mt_status mt_resolve_positions_device(mt_engine* e, const mt_pos_query* d_q, uint32_t n, mt_pos_result* d_out) {
    if (!e || (n && (!d_q || !d_out))) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_resolve(&e->g, d_q, n, e->n_docs, d_out, e->stream));
    return MT_OK;
}

mt_status mt_marker_positions(mt_engine* e, const mt_marker_query* q, uint32_t n, mt_marker_result* out) {
    static_assert(sizeof(mt_marker_query) == 16 && sizeof(mt_marker_result) == 16, "mt_marker_query / result are 16 bytes");
    if (!e || (n && (!q || !out)) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    for (uint32_t i = 0; i < n; i++)
        if (q[i].key >= MT_MAX_KEYS_WIDE) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, dr] = s.carve<mt_marker_query, mt_marker_result>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_marker_positions, &e->g, dq, n, e->n_docs, dr, e->stream)
        .d2h(out, dr, n * sizeof *out)
        .sync().status();
}

mt_status mt_marker_positions_device(mt_engine* e, const mt_marker_query* d_q, uint32_t n, mt_marker_result* d_out) {
    if (!e || (n && (!d_q || !d_out))) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_marker_positions(&e->g, d_q, n, e->n_docs, d_out, e->stream));
    return MT_OK;
}

mt_status mt_segment_infos(mt_engine* e, const uint32_t* docs, const int32_t* ordinals, uint32_t n, mt_seg_info* out) {
    static_assert(sizeof(mt_seg_info) == 168, "mt_seg_info is 168 bytes");
    if (!e || (n && (!docs || !ordinals || !out)) || !mt_docs_below(docs, n, e->n_docs)) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dd, dor, dout] = s.carve<uint32_t, int32_t, mt_seg_info>(n, n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dd, docs, n * sizeof *docs)
        .h2d(dor, ordinals, n * sizeof *ordinals)
        .launch(mt_launch_seginfo, &e->g, dd, dor, n, dout, e->stream)
        .d2h(out, dout, n * sizeof *out)
        .sync().status();
}

mt_status mt_segment_text(mt_engine* e, uint32_t doc, uint32_t toff, uint32_t len, uint16_t* out) {
    if (!e || doc >= e->n_docs || (len && !out)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_doc_scalars sc;
    HIP_OK(hipMemcpyAsync(&sc, e->g.sc + doc, sizeof sc, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if ((uint64_t)toff + len > sc.text_top) return MT_ERR_ARG;
    if (!len) return MT_OK;
    const size_t base = ((size_t)doc * 2 + sc.text_half) * e->g.textcap;
    if (sc.wide & MT_WIDE_DOC) {
        HIP_OK(hipMemcpy(out, e->g.text + base + (size_t)toff * 2, (size_t)len * 2, hipMemcpyDeviceToHost));
        return MT_OK;
    }
    std::vector<uint8_t> b(len);
    HIP_OK(hipMemcpy(b.data(), e->g.text + base + toff, len, hipMemcpyDeviceToHost));
    for (uint32_t i = 0; i < len; i++) out[i] = b[i];
    return MT_OK;
}

mt_status mt_regen_drain(mt_engine* e, uint32_t doc, mt_op_rec* recs, uint32_t cap, uint8_t* payload, uint32_t pcap,
                         uint32_t* n, uint32_t* pn) {
    if (!e || doc >= e->n_docs || !n || !pn) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(hipStreamSynchronize(e->stream));
    uint32_t cnt[2] = {0, 0};  // mt_loc::rgn, rgpn (adjacent)
    HIP_OK(hipMemcpy(cnt, &e->g.loc[doc].rgn, sizeof cnt, hipMemcpyDeviceToHost));
    *n = cnt[0];
    *pn = cnt[1];
    if (!recs) return MT_OK;  // sizes only
    // a drain takes everything or nothing: buffers too small leave the records in place
    if (cap < cnt[0] || (cnt[1] && (!payload || pcap < cnt[1]))) return MT_ERR_ARG;
    if (cnt[0])
        HIP_OK(hipMemcpy(recs, e->g.rg + (size_t)doc * MT_RG_RECS, cnt[0] * sizeof(mt_op_rec), hipMemcpyDeviceToHost));
    if (cnt[1]) HIP_OK(hipMemcpy(payload, e->g.rgp + (size_t)doc * MT_RG_BYTES, cnt[1], hipMemcpyDeviceToHost));
    HIP_OK(hipMemset(&e->g.loc[doc].rgn, 0, sizeof cnt));
    e->gen++;  // (the regenerated ops are document state: mt_docs_save)
    return MT_OK;
}

mt_status mt_range_stacks(mt_engine* e, const mt_tile_query* q, uint32_t n, uint32_t cap, mt_stack_item* items,
                          uint32_t* depth) {
    static_assert(sizeof(mt_stack_item) == 12, "mt_stack_item is 12 bytes");
    if (!e || (n && (!q || !depth || (cap && !items))) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, di, dd] = s.carve<mt_tile_query, mt_stack_item, uint32_t>(n, (size_t)n * cap, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_stacks, &e->g, dq, n, cap, di, dd, e->stream)
        .d2h(items, di, (size_t)n * cap * sizeof(mt_stack_item))
        .d2h(depth, dd, n * sizeof *depth)
        .sync().status();
}

mt_status mt_events_enable(mt_engine* e, uint32_t per_doc) {
    static_assert(sizeof(mt_event) == 96, "mt_event is 96 bytes");
    if (!e) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (e->g.ev) HIP_OK(hipFree(e->g.ev));
    if (e->g.evn) HIP_OK(hipFree(e->g.evn));
    refs_free(e);  // (they follow this buffer's rows)
    e->g.ev = nullptr;
    e->g.evn = nullptr;
    e->g.evcap = 0;
    // the register engine records events in its own kernels (mtr::reg_apply_kernel_ev; its C64
    // documents on the LDS engine); MTGPU_EV_ENGINE=lds keeps every class on the LDS engine instead
    const char* evw = getenv("MTGPU_EV_ENGINE");
    e->use_reg = (per_doc && evw && strcmp(evw, "lds") == 0) ? false : e->reg_default;
    e->first_lds = e->use_reg ? kFirstLds : 0;
    if (!per_doc) return MT_OK;
    const size_t D = e->cfg.max_docs;
    if (hipMalloc(&e->g.ev, D * per_doc * sizeof(mt_event)) != hipSuccess ||
        hipMalloc(&e->g.evn, D * sizeof(uint32_t)) != hipSuccess) {
        if (e->g.ev) (void)hipFree(e->g.ev);
        e->g.ev = nullptr;
        e->g.evn = nullptr;
        e->use_reg = e->reg_default;
        e->first_lds = e->use_reg ? kFirstLds : 0;
        return MT_ERR_NOMEM;
    }
    e->g.evcap = per_doc;
    HIP_OK(hipMemset(e->g.evn, 0, D * sizeof(uint32_t)));
    return MT_OK;
}

mt_status mt_events_drain(mt_engine* e, mt_event* out, uint64_t cap, uint32_t* row_ptr, uint64_t* total) {
    if (!e || !row_ptr || !total || !e->g.ev) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    if (out) HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));  // the rows move the references first
    HIP_OK(hipStreamSynchronize(e->stream));
    const uint32_t n = e->n_docs;
    std::vector<uint32_t> cnt(n);
    if (n) HIP_OK(hipMemcpy(cnt.data(), e->g.evn, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    std::vector<uint64_t> off(n + 1, 0);
    for (uint32_t d = 0; d < n; d++) off[d + 1] = off[d] + std::min(cnt[d], e->g.evcap);
    if (off[n] >= (1ull << 32)) return MT_ERR_ARG;
    for (uint32_t d = 0; d <= n; d++) row_ptr[d] = (uint32_t)off[d];
    *total = off[n];
    if (!out) return MT_OK;
    if (cap < off[n]) return MT_ERR_ARG;
    if (off[n]) {
        mt_scratch s;
        auto [d_off, d_out] = s.carve<uint64_t, mt_event>(off.size(), off[n]);
        const mt_status st = mt_chain(e->stream, s.status())
                                 .h2d(d_off, off.data(), off.size() * sizeof(uint64_t))
                                 .launch(mt_launch_events_pack, &e->g, n, d_off, d_out, e->stream)
                                 .d2h(out, d_out, off[n] * sizeof(mt_event))
                                 .sync().status();
        if (st) return st;
    }
    mt_chain c(e->stream);
    c.launch(hipMemsetAsync, e->g.evn, 0, (size_t)n * sizeof(uint32_t), e->stream);
    if (e->g.refcur) c.launch(hipMemsetAsync, e->g.refcur, 0, (size_t)n * sizeof(uint32_t), e->stream);
    return c.sync().status();
}

// ---- local references (include/mtgpu.h; kernels in mt_refs.hip) ---------------------------------
mt_status mt_refs_enable(mt_engine* e, uint32_t per_doc) {
    static_assert(sizeof(mt_ref) == 16 && sizeof(mt_ref_add) == 12 && sizeof(mt_ref_pos) == 12, "reference records");
    if (!e || (per_doc && !e->g.ev) || per_doc > MT_REFS_MAX) return MT_ERR_ARG;  // (the fold stages a table in LDS)
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(hipStreamSynchronize(e->stream));
    refs_free(e);
    if (!per_doc) return MT_OK;
    const size_t D = e->cfg.max_docs;
    if (hipMalloc(&e->g.refs, D * 2 * per_doc * sizeof(mt_ref)) != hipSuccess ||
        hipMalloc(&e->g.refpos, D * per_doc * sizeof(mt_ref_pos)) != hipSuccess ||
        hipMalloc(&e->g.refcur, D * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&e->g.refn, D * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&e->g.refq, D * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&e->g.refdrop, D * sizeof(uint32_t)) != hipSuccess) {
        refs_free(e);
        return MT_ERR_NOMEM;
    }
    e->g.refcap = per_doc;
    HIP_OK(refs_clear(e));
    // (rows recorded before now concern no reference: the first fold only moves the cursors past them)
    HIP_OK(hipStreamSynchronize(e->stream));
    return MT_OK;
}

mt_status mt_refs_add(mt_engine* e, const mt_ref_add* in, uint32_t n, uint32_t* handles) {
    if (!e || !e->g.refs || (n && (!in || !handles)) || !mt_docs_below(in, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    if (n == 0) return MT_OK;
    e->gen++;
    std::vector<mt_pos_query> q(n);
    for (uint32_t i = 0; i < n; i++) q[i] = mt_pos_query{in[i].doc, in[i].pos, MT_POS_LOCAL, 0, MT_POS_CONTAINING};
    mt_scratch s;
    auto [da, dq, dr, dh] = s.carve<mt_ref_add, mt_pos_query, mt_pos_result, uint32_t>(n, n, n, n);
    return mt_chain(e->stream, s.status())
        .h2d(da, in, n * sizeof *in)
        .h2d(dq, q.data(), n * sizeof(mt_pos_query))
        .launch(mt_launch_resolve, &e->g, dq, n, e->n_docs, dr, e->stream)
        .launch(mt_launch_refs_claim, &e->g, da, dr, n, e->n_docs, dh, e->stream)
        .d2h(handles, dh, n * sizeof *handles)
        .sync().status();
}

mt_status mt_refs_remove(mt_engine* e, const uint32_t* docs, const uint32_t* handles, uint32_t n) {
    if (!e || !e->g.refs || (n && (!docs || !handles)) || !mt_docs_below(docs, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    if (n == 0) return MT_OK;
    e->gen++;
    mt_scratch s;
    auto [dd, dh] = s.carve<uint32_t, uint32_t>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dd, docs, n * sizeof *docs)
        .h2d(dh, handles, n * sizeof *handles)
        .launch(mt_launch_refs_release, &e->g, dd, dh, n, e->n_docs, e->stream)
        .sync().status();
}

mt_status mt_refs_dropped(mt_engine* e, uint32_t* out, uint32_t n_docs) {
    if (!e || !e->g.refs || !out || n_docs > e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (n_docs) HIP_OK(hipMemcpy(out, e->g.refdrop, (size_t)n_docs * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return MT_OK;
}

mt_status mt_refs_positions_device(mt_engine* e, const uint32_t* d_docs, const uint32_t* d_handles, uint32_t n,
                                   mt_ref_pos* d_out) {
    if (!e || !e->g.refs || (n && (!d_docs || !d_handles || !d_out))) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    HIP_OK(mt_launch_refs_positions(&e->g, d_docs, d_handles, n, e->n_docs, d_out, e->stream));
    return MT_OK;
}

mt_status mt_refs_positions(mt_engine* e, const uint32_t* docs, const uint32_t* handles, uint32_t n, mt_ref_pos* out) {
    if (!e || !e->g.refs || (n && (!docs || !handles || !out)) || !mt_docs_below(docs, n, e->n_docs))
        return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    if (n == 0) return mt_refs_positions_device(e, nullptr, nullptr, 0, nullptr);
    mt_scratch s;
    auto [dd, dh, dout] = s.carve<uint32_t, uint32_t, mt_ref_pos>(n, n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dd, docs, n * sizeof *docs)
        .h2d(dh, handles, n * sizeof *handles)
        .call(mt_refs_positions_device, e, dd, dh, n, dout)
        .d2h(out, dout, n * sizeof *out)
        .sync().status();
}

mt_status mt_refs_insert_local(mt_engine* e, const mt_ref_insert* at, const mt_op_rec* ops, uint32_t n,
                               const uint8_t* payload, uint64_t payload_bytes, int32_t* positions) {
    static_assert(sizeof(mt_ref_insert) == 8, "mt_ref_insert is 8 bytes");
    if (!e || !e->g.refs || (n && (!at || !ops || !positions)) || (payload_bytes && !payload)) return MT_ERR_ARG;
    std::vector<uint32_t> rows((size_t)e->n_docs + 1);
    if (!mt_ref_insert_rows(at, ops, n, e->n_docs, payload_bytes, rows.data())) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    std::vector<uint32_t> docs(n), handles(n);
    for (uint32_t i = 0; i < n; i++) {
        docs[i] = at[i].doc;
        handles[i] = at[i].handle;
    }
    mt_scratch s;
    auto [dd, dh, dat, dops, dpay, drows, dpos] = s.carve<uint32_t, uint32_t, mt_ref_pos, mt_op_rec, uint8_t, uint32_t, int32_t>(
        n, n, n, n, std::max<uint64_t>(1, payload_bytes), rows.size(), n);
    mt_batch b;
    b.ops = dops;
    b.payload = dpay;
    b.row_ptr = drows;
    b.n_ops = n;
    b.payload_bytes = payload_bytes;
    b.n_docs = e->n_docs;
    b.max_ops_per_doc = 1;
    return mt_chain(e->stream, s.status())
        .h2d(dd, docs.data(), n * sizeof(uint32_t))
        .h2d(dh, handles.data(), n * sizeof(uint32_t))
        .h2d(dops, ops, n * sizeof *ops)
        .h2d(dpay, payload, payload_bytes)
        .h2d(drows, rows.data(), rows.size() * sizeof(uint32_t))
        .call(mt_refs_positions_device, e, dd, dh, n, dat)
        .launch(mt_launch_refs_stamp, &e->g, dd, dat, dops, n, e->n_docs, dpos, e->stream)
        .d2h(positions, dpos, n * sizeof *positions)
        .call(mt_batch_apply, e, &b)
        .sync().status();
}

// ---- interval collections (include/mtgpu.h; kernels in mt_intervals.hip) -------------------------
mt_status mt_intervals_enable(mt_engine* e, uint32_t per_doc) {
    static_assert(sizeof(mt_interval) == 16 && sizeof(mt_interval_add) == 16 && sizeof(mt_interval_query) == 16 &&
                      sizeof(mt_interval_pos) == 24,
                  "interval records");
    if (!e || (per_doc && (!e->g.refs || 2ull * per_doc > e->g.refcap))) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(hipStreamSynchronize(e->stream));
    intervals_free(e);
    if (!per_doc) return MT_OK;
    const size_t D = e->cfg.max_docs;
    if (hipMalloc(&e->g.ivs, D * per_doc * sizeof(mt_interval)) != hipSuccess ||
        hipMalloc(&e->g.ivn, D * sizeof(uint32_t)) != hipSuccess) {
        intervals_free(e);
        return MT_ERR_NOMEM;
    }
    e->g.ivcap = per_doc;
    HIP_OK(mt_launch_intervals_free_docs(&e->g, nullptr, e->cfg.max_docs, e->cfg.max_docs, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return MT_OK;
}

mt_status mt_intervals_add(mt_engine* e, const mt_interval_add* in, uint32_t n, uint32_t* handles) {
    if (!e || !e->g.ivs || (n && (!in || !handles)) || !mt_docs_below(in, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    if (n == 0) return MT_OK;
    e->gen++;
    std::vector<mt_pos_query> q(2 * (size_t)n);
    for (uint32_t i = 0; i < n; i++) {
        q[2 * i] = mt_pos_query{in[i].doc, in[i].start, MT_POS_LOCAL, 0, MT_POS_CONTAINING};
        q[2 * i + 1] = mt_pos_query{in[i].doc, in[i].end, MT_POS_LOCAL, 0, MT_POS_CONTAINING};
    }
    mt_scratch s;
    auto [da, dq, dr, dh] = s.carve<mt_interval_add, mt_pos_query, mt_pos_result, uint32_t>(n, q.size(), q.size(), n);
    return mt_chain(e->stream, s.status())
        .h2d(da, in, n * sizeof *in)
        .h2d(dq, q.data(), q.size() * sizeof(mt_pos_query))
        .launch(mt_launch_resolve, &e->g, dq, 2 * n, e->n_docs, dr, e->stream)
        .launch(mt_launch_intervals_claim, &e->g, da, dr, n, e->n_docs, dh, e->stream)
        .d2h(handles, dh, n * sizeof *handles)
        .sync().status();
}

mt_status mt_intervals_remove(mt_engine* e, const mt_interval_query* q, uint32_t n, uint32_t* removed) {
    if (!e || !e->g.ivs || (n && (!q || !removed)) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    if (n == 0) return MT_OK;
    e->gen++;
    mt_scratch s;
    auto [dq, dh] = s.carve<mt_interval_query, uint32_t>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_intervals_release, &e->g, dq, n, e->n_docs, dh, e->stream)
        .d2h(removed, dh, n * sizeof *removed)
        .sync().status();
}

mt_status mt_intervals_overlapping_device(mt_engine* e, const mt_interval_query* d_q, uint32_t n,
                                          const uint32_t* d_row_ptr, uint32_t* d_counts, uint32_t* d_out) {
    if (!e || !e->g.ivs || (n && (!d_q || !d_counts || (d_row_ptr && !d_out)))) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    HIP_OK(mt_launch_intervals_overlap(&e->g, d_q, n, e->n_docs, d_row_ptr, d_counts, d_out, e->stream));
    return MT_OK;
}

// The two-pass readers (this one and mt_text_ranges): the count pass, the rows' prefix sums on the
// host (a sum reaching 2^32 is refused), the sizing call's return, the capacity check, then the write
// pass into a second block of exactly the answer's size.
mt_status mt_intervals_overlapping(mt_engine* e, const mt_interval_query* q, uint32_t n, uint32_t* row_ptr,
                                   uint32_t* out, uint64_t cap, uint64_t* total) {
    if (!e || !e->g.ivs || !row_ptr || !total || (n && !q) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    row_ptr[0] = 0;
    *total = 0;
    if (n == 0) return mt_intervals_overlapping_device(e, nullptr, 0, nullptr, nullptr, nullptr);
    mt_scratch s;
    auto [dq, dc, drp] = s.carve<mt_interval_query, uint32_t, uint32_t>(n, n, (size_t)n + 1);
    std::vector<uint32_t> cnt(n);
    const mt_status st = mt_chain(e->stream, s.status())
                             .h2d(dq, q, n * sizeof *q)
                             .call(mt_intervals_overlapping_device, e, dq, n, nullptr, dc, nullptr)
                             .d2h(cnt.data(), dc, n * sizeof(uint32_t))
                             .sync().status();
    if (st) return st;
    if (!mt_rows_from_counts(n, [&](uint32_t i) { return cnt[i]; }, row_ptr, total)) return MT_ERR_ARG;
    if (!out || *total == 0) return MT_OK;
    if (cap < *total) return MT_ERR_ARG;
    mt_scratch so;
    auto [dout] = so.carve<uint32_t>(*total);
    return mt_chain(e->stream, so.status())
        .h2d(drp, row_ptr, ((size_t)n + 1) * sizeof(uint32_t))
        .call(mt_intervals_overlapping_device, e, dq, n, drp, dc, dout)
        .d2h(out, dout, *total * sizeof(uint32_t))
        .sync().status();
}

mt_status mt_text_ranges_device(mt_engine* e, const mt_text_query* d_q, uint32_t n, const uint32_t* d_row_ptr,
                                uint16_t* d_units, const uint32_t* d_m_row_ptr, mt_text_marker* d_markers,
                                mt_text_count* d_counts) {
    static_assert(sizeof(mt_text_query) == 32 && sizeof(mt_text_marker) == 8 && sizeof(mt_text_count) == 8,
                  "mt_text_query is 32 bytes, mt_text_marker and mt_text_count 8");
    if (!e || (n && (!d_q || !d_counts || (d_row_ptr && !d_units) || (d_m_row_ptr && (!d_row_ptr || !d_markers)))))
        return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_text_ranges(&e->g, d_q, n, e->n_docs, d_row_ptr, d_units, d_m_row_ptr, d_markers, d_counts, e->stream));
    return MT_OK;
}

mt_status mt_text_lengths(mt_engine* e, const mt_text_query* q, uint32_t n, mt_text_count* out) {
    if (!e || (n && (!q || !out)) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, dc] = s.carve<mt_text_query, mt_text_count>(n, n);
    return mt_chain(e->stream, s.status())
        .h2d(dq, q, n * sizeof *q)
        .launch(mt_launch_text_ranges, &e->g, dq, n, e->n_docs, nullptr, nullptr, nullptr, nullptr, dc, e->stream)
        .d2h(out, dc, n * sizeof *out)
        .sync().status();
}

mt_status mt_text_ranges(mt_engine* e, const mt_text_query* q, uint32_t n, uint32_t* row_ptr, uint16_t* units,
                         uint64_t cap, uint32_t* m_row_ptr, mt_text_marker* markers, uint64_t m_cap, uint64_t* totals) {
    if (!e || !row_ptr || !m_row_ptr || !totals || (n && !q) || !mt_docs_below(q, n, e->n_docs)) return MT_ERR_ARG;
    row_ptr[0] = m_row_ptr[0] = 0;
    totals[0] = totals[1] = 0;
    if (n == 0) return MT_OK;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [dq, dc, drp, dmrp] = s.carve<mt_text_query, mt_text_count, uint32_t, uint32_t>(n, n, (size_t)n + 1, (size_t)n + 1);
    std::vector<mt_text_count> cnt(n);
    const mt_status st = mt_chain(e->stream, s.status())
                             .h2d(dq, q, n * sizeof *q)
                             .call(mt_text_ranges_device, e, dq, n, nullptr, nullptr, nullptr, nullptr, dc)
                             .d2h(cnt.data(), dc, n * sizeof(mt_text_count))
                             .sync().status();
    if (st) return st;
    uint64_t sum = 0, msum = 0;
    if (!mt_rows_from_counts(n, [&](uint32_t i) { return cnt[i].units; }, row_ptr, &sum) ||
        !mt_rows_from_counts(n, [&](uint32_t i) { return cnt[i].markers; }, m_row_ptr, &msum))
        return MT_ERR_ARG;
    totals[0] = sum;
    totals[1] = msum;
    if (!units || sum + msum == 0) return MT_OK;
    if (cap < sum || m_cap < msum || (msum && !markers)) return MT_ERR_ARG;
    mt_scratch so;
    auto [du, dm] = so.carve<uint16_t, mt_text_marker>(sum, msum);
    return mt_chain(e->stream, so.status())
        .h2d(drp, row_ptr, ((size_t)n + 1) * sizeof(uint32_t))
        .h2d(dmrp, m_row_ptr, ((size_t)n + 1) * sizeof(uint32_t))
        .call(mt_text_ranges_device, e, dq, n, drp, du, dmrp, dm, dc)
        .d2h(units, du, sum * sizeof(uint16_t))
        .d2h(markers, dm, msum * sizeof(mt_text_marker))
        .sync().status();
}

mt_status mt_intervals_positions(mt_engine* e, const uint32_t* docs, uint32_t n, mt_interval_pos* out) {
    if (!e || !e->g.ivs || (n && (!docs || !out)) || !mt_docs_below(docs, n, e->n_docs)) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HIP_OK(mt_launch_refs_track(&e->g, e->n_docs, e->stream));
    if (n == 0) return MT_OK;
    mt_scratch s;
    auto [dd, dout] = s.carve<uint32_t, mt_interval_pos>(n, (size_t)n * e->g.ivcap);
    return mt_chain(e->stream, s.status())
        .h2d(dd, docs, n * sizeof *docs)
        .launch(mt_launch_refs_resolve_docs, &e->g, dd, n, e->n_docs, e->stream)
        .launch(mt_launch_intervals_gather, &e->g, dd, n, e->n_docs, dout, e->stream)
        .d2h(out, dout, (size_t)n * e->g.ivcap * sizeof(mt_interval_pos))
        .sync().status();
}

mt_status mt_checksums_device(mt_engine* e, uint64_t* d_out, uint32_t n_docs) {
    if (!e || !d_out || n_docs > e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    if (!n_docs) return MT_OK;
    HIP_OK(mt_launch_checksum(&e->g, n_docs, d_out, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    return MT_OK;
}

mt_status mt_checksums(mt_engine* e, uint64_t* out, uint32_t n_docs) {
    if (!e || !out || n_docs > e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_scratch s;
    auto [d] = s.carve<uint64_t>(n_docs);
    return mt_chain(e->stream, s.status())
        .launch(mt_launch_checksum, &e->g, n_docs, d, e->stream)
        .d2h(out, d, n_docs * sizeof(uint64_t))
        .sync().status();
}

mt_status mt_seg_counts(mt_engine* e, uint32_t* out, uint32_t n_docs) {
    if (!e || !out || n_docs > e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    std::vector<mt_doc_scalars> sc(n_docs);
    HIP_OK(hipMemcpyAsync(sc.data(), e->g.sc, n_docs * sizeof(mt_doc_scalars), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    for (uint32_t d = 0; d < n_docs; d++) out[d] = (uint32_t)sc[d].nseg;
    return MT_OK;
}

mt_status mt_doc_error(mt_engine* e, uint32_t doc, int32_t* code, int32_t* seq) {
    if (!e || doc >= e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    mt_doc_scalars sc;
    HIP_OK(hipMemcpyAsync(&sc, e->g.sc + doc, sizeof sc, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (code) *code = sc.err;
    if (seq) *seq = sc.err_seq;
    return MT_OK;
}

}  // extern "C"
