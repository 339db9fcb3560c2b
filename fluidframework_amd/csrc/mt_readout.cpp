// mt_readout.cpp -- the canonical readout of libmtgpu.so (include/mtgpu.h): a document's state
// fetched to the host (HostDoc), its state JSON, the SnapshotV1 emit over the device's extraction
// specs, text and length.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "mt_checksum.h"
#include "mt_engine_impl.h"
#include "mt_scratch.h"

namespace {
// A document's state on the host, narrow or wide (mt_state.h): text as UTF-16 code units, props as
// a value id per key, overlap as a sorted client list
struct HostDoc {
    mt_doc_scalars sc;
    bool wide = false;
    std::vector<int32_t> seq, rseq;
    std::vector<uint32_t> len, toff;
    std::vector<uint64_t> ovl, props, ovx, ph, pxl, pxh, pxx;
    std::vector<uint8_t> client, rclient, flags;
    std::vector<uint16_t> chi;                 // (wide) the short ids' high bytes
    std::vector<uint16_t> text;                // the arena's current half, in code units
    std::vector<std::vector<uint8_t>> levels;  // per level child counts (level 0 = leaf blocks)
    uint32_t prop(int i, int k) const {
        const int sh = 8 * (k & 7);
        if (!wide) return k < 8 ? (uint32_t)((props[i] >> sh) & 0xFF) : 0u;
        if (k >= 16 && !(sc.wide & MT_WIDE_XKV)) return 0u;  // (no keys 16..31 stored)
        const uint64_t lo = k < 8 ? props[i] : k < 16 ? pxl[i] : pxx[4 * (size_t)i + 2 * ((k - 16) >> 3)];
        const uint64_t hi = k < 8 ? ph[i] : k < 16 ? pxh[i] : pxx[4 * (size_t)i + 2 * ((k - 16) >> 3) + 1];
        return (uint32_t)((lo >> sh) & 0xFF) | ((uint32_t)((hi >> sh) & 0xFF) << 8);
    }
    std::vector<int> overlap(int i) const {
        std::vector<int> v;
        for (int c = 0; c < 64; c++)
            if ((ovl[i] >> c) & 1) v.push_back(c);
        if (wide) {
            const uint64_t* x = ovx.data() + (size_t)MT_OVX_WORDS * i;
            for (int q = 0; q < MT_OVX_IDS; q++) {
                const int c = (int)mt_ovx_id2(x, (sc.wide & MT_WIDE_XOV) ? x + 4 : nullptr, q);
                if (!c) break;
                v.push_back(c);
            }
        }
        return v;
    }
    uint32_t client_of(int i) const { return client[i] | (wide ? (uint32_t)(chi[i] & 0xFF) << 8 : 0u); }
    uint32_t rclient_of(int i) const { return rclient[i] | (wide ? (uint32_t)(chi[i] >> 8) << 8 : 0u); }
    const uint16_t* units(int i) const { return text.data() + toff[i]; }
};

template <class T>
hipError_t fetch(std::vector<T>& v, const T* base, size_t off, size_t n, hipStream_t st) {
    v.resize(n);
    if (!n) return hipSuccess;
    return hipMemcpyAsync(v.data(), base + off, n * sizeof(T), hipMemcpyDeviceToHost, st);
}

// the current arena half of document d as code units (a narrow document's bytes widened)
mt_status fetch_text(mt_engine* e, uint32_t d, const mt_doc_scalars& sc, std::vector<uint16_t>& out) {
    const mt_gstate& g = e->g;
    const size_t base = ((size_t)d * 2 + sc.text_half) * g.textcap;
    if (sc.wide & MT_WIDE_DOC) {
        out.resize(sc.text_top);
        if (sc.text_top)
            HIP_OK(hipMemcpyAsync(out.data(), g.text + base, (size_t)sc.text_top * 2, hipMemcpyDeviceToHost, e->stream));
        HIP_OK(hipStreamSynchronize(e->stream));
        return MT_OK;
    }
    std::vector<uint8_t> b;
    HIP_OK(fetch(b, g.text, base, sc.text_top, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    out.assign(b.begin(), b.end());
    return MT_OK;
}

mt_status read_doc(mt_engine* e, uint32_t d, HostDoc& h) {
    const mt_gstate& g = e->g;
    HIP_OK(hipMemcpyAsync(&h.sc, g.sc + d, sizeof h.sc, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    h.wide = (h.sc.wide & MT_WIDE_DOC) != 0 && g.ovx;
    const size_t so = (size_t)d * g.segcap, n = (size_t)h.sc.nseg;
    HIP_OK(fetch(h.seq, g.seq, so, n, e->stream));
    HIP_OK(fetch(h.rseq, g.rseq, so, n, e->stream));
    HIP_OK(fetch(h.len, g.len, so, n, e->stream));
    HIP_OK(fetch(h.toff, g.toff, so, n, e->stream));
    HIP_OK(fetch(h.ovl, g.ovl, so, n, e->stream));
    HIP_OK(fetch(h.props, g.props, so, n, e->stream));
    if (h.wide) {
        HIP_OK(fetch(h.ovx, g.ovx, so * MT_OVX_WORDS, n * MT_OVX_WORDS, e->stream));
        HIP_OK(fetch(h.chi, g.chi, so, n, e->stream));
        HIP_OK(fetch(h.ph, g.ph, so, n, e->stream));
        HIP_OK(fetch(h.pxl, g.pxl, so, n, e->stream));
        HIP_OK(fetch(h.pxh, g.pxh, so, n, e->stream));
        HIP_OK(fetch(h.pxx, g.pxx, so * 4, n * 4, e->stream));
    }
    HIP_OK(fetch(h.client, g.client, so, n, e->stream));
    HIP_OK(fetch(h.rclient, g.rclient, so, n, e->stream));
    HIP_OK(fetch(h.flags, g.flags, so, n, e->stream));
    h.levels.resize(h.sc.nlev);
    for (int L = 0; L < h.sc.nlev; L++) {
        if (L == 0) HIP_OK(fetch(h.levels[0], g.lbcnt, (size_t)d * g.lbcap, h.sc.nb[0], e->stream));
        else HIP_OK(fetch(h.levels[L], g.ibcnt, ((size_t)d * (MT_MAXLEV - 1) + (L - 1)) * g.ibcap, h.sc.nb[L], e->stream));
    }
    HIP_OK(hipStreamSynchronize(e->stream));
    return fetch_text(e, d, h.sc, h.text);
}

// A JSON string of UTF-16 code units, ASCII only: printable ASCII as itself, \" \\ and the short
// forms JSON.stringify uses (ECMA-262 QuoteJSONString), every other unit -- non-ASCII and surrogate
// halves included -- as \uXXXX.  It parses to the same string the reference's JSON holds.
void json_units(std::string& o, const uint16_t* p, size_t n) {
    o += '"';
    for (size_t i = 0; i < n; i++) {
        const unsigned c = p[i];
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\b': o += "\\b"; break;
            case '\t': o += "\\t"; break;
            case '\n': o += "\\n"; break;
            case '\f': o += "\\f"; break;
            case '\r': o += "\\r"; break;
            default:
                if (c < 0x20 || c >= 0x7F) {
                    char buf[8];
                    snprintf(buf, sizeof buf, "\\u%04x", c);
                    o += buf;
                } else {
                    o += (char)c;
                }
        }
    }
    o += '"';
}

std::string state_json(const HostDoc& h) {
    std::string o = "{\"seq\":" + std::to_string(h.sc.cur_seq) + ",\"msn\":" + std::to_string(h.sc.min_seq) + ",\"segs\":[";
    for (int i = 0; i < h.sc.nseg; i++) {
        if (i) o += ',';
        o += '[';
        if (h.flags[i] & MT_SF_MARKER)  // a Marker: {"marker": refType}
            o += "{\"marker\":" + std::to_string(h.units(i)[0]) + "}";
        else
            json_units(o, h.units(i), h.len[i]);
        const bool rm = h.flags[i] & MT_SF_REMOVED;
        o += ',' + std::to_string(h.seq[i]) + ',' + std::to_string(mt_canon_client(h.client_of(i))) + ',';
        o += (rm ? std::to_string(h.rseq[i]) : "-1") + ',' + (rm ? std::to_string(h.rclient_of(i)) : "-1") + ",[";
        bool f = true;
        for (int c : h.overlap(i)) {
            if (!f) o += ',';
            f = false;
            o += std::to_string(c);
        }
        o += "],";
        if (!(h.flags[i] & MT_SF_PDEF)) {
            o += "null";
        } else {
            o += '{';
            bool f2 = true;
            for (int k = 0; k < MT_MAX_KEYS_WIDE; k++) {
                const unsigned v = h.prop(i, k);
                if (!v) continue;
                if (!f2) o += ',';
                f2 = false;
                o += "\"k" + std::to_string(k) + "\":" + std::to_string(v);
            }
            o += '}';
        }
        o += ']';
    }
    o += "],\"tree\":[";
    for (int depth = 0; depth < h.sc.nlev; depth++) {
        const auto& lv = h.levels[h.sc.nlev - 1 - depth];
        if (depth) o += ',';
        o += '[';
        for (size_t b = 0; b < lv.size(); b++) {
            if (b) o += ',';
            o += std::to_string(lv[b]);
        }
        o += ']';
    }
    o += "]}";
    return o;
}

// props as the reference's map: keys "k<id>" (interned key ids), values = interned value ids
void props_json(std::string& o, const HostDoc& h, int i) {
    o += '{';
    bool first = true;
    for (int k = 0; k < MT_MAX_KEYS_WIDE; k++) {
        const unsigned v = h.prop(i, k);
        if (!v) continue;
        if (!first) o += ',';
        first = false;
        o += "\"k" + std::to_string(k) + "\":" + std::to_string(v);
    }
    o += '}';
}

// TextSegment.toJSONObject (textSegment.ts:47-53) of `text` with the props of segment i;
// Marker.toJSONObject (mergeTree.ts:652-656) for a marker: {marker: {refType}, props?}
void seg_json(std::string& o, const HostDoc& h, int i, const std::vector<uint16_t>& text) {
    if (h.flags[i] & MT_SF_MARKER) {
        o += "{\"marker\":{\"refType\":" + std::to_string(h.units(i)[0]) + "}";
        if (h.flags[i] & MT_SF_PDEF) {
            o += ",\"props\":";
            props_json(o, h, i);
        }
        o += '}';
    } else if (h.flags[i] & MT_SF_PDEF) {
        o += "{\"text\":";
        json_units(o, text.data(), text.size());
        o += ",\"props\":";
        props_json(o, h, i);
        o += '}';
    } else {
        json_units(o, text.data(), text.size());
    }
}

std::string client_name(const char* const* names, uint32_t n_names, uint32_t c) {
    if (c == MT_CLIENT_NONCOLLAB) return "original";  // Client.getLongClientId of a negative id (client.ts:645-652)
    if (names && c < n_names && names[c]) return names[c];
    return std::to_string(c);
}

// SnapshotV1.emit (snapshotV1.ts:85-149) from the device's extraction specs: the tree entries as
// one JSON object {"header": chunk, "body_0": chunk, ...}
std::string snapshot_json(const HostDoc& h, const std::vector<uint32_t>& sp, uint32_t nspec, uint32_t chunk,
                          const char* const* names, uint32_t n_names) {
    std::vector<std::string> specs(nspec);
    std::vector<uint32_t> lens(nspec);
    for (uint32_t k = 0; k < nspec; k++) {
        const int pos = (int)sp[3 * k];
        const int cnt = (int)(sp[3 * k + 1] >> 1);
        const bool meta = sp[3 * k + 1] & 1u;
        std::vector<uint16_t> text;
        for (int i = pos; i < pos + cnt; i++) {
            // elided inside the run: removed at or below the MSN, or a pending local insert / removal
            if (h.seq[i] == -1 || ((h.flags[i] & MT_SF_REMOVED) && h.rseq[i] <= h.sc.min_seq)) continue;
            text.insert(text.end(), h.units(i), h.units(i) + h.len[i]);
        }
        lens[k] = sp[3 * k + 2];
        std::string& o = specs[k];
        if (!meta) {
            seg_json(o, h, pos, text);
            continue;
        }
        o += "{\"json\":";
        seg_json(o, h, pos, text);
        if (h.seq[pos] > h.sc.min_seq)
            o += ",\"seq\":" + std::to_string(h.seq[pos]) + ",\"client\":\"" + client_name(names, n_names, h.client_of(pos)) +
                 "\"";
        if (h.flags[pos] & MT_SF_REMOVED)
            o += ",\"removedSeq\":" + std::to_string(h.rseq[pos]) + ",\"removedClient\":\"" +
                 client_name(names, n_names, h.rclient_of(pos)) + "\"";
        o += '}';
    }
    // getSeqLengthSegs (:57-79): chunks of >= `chunk` characters
    struct Chunk { uint32_t start, count; uint64_t length; };
    std::vector<Chunk> chunks;
    uint32_t total_count = 0;
    uint64_t total_len = 0;
    do {
        Chunk c{total_count, 0, 0};
        while (c.length < chunk && c.start + c.count < nspec) c.length += lens[c.start + c.count++];
        chunks.push_back(c);
        total_count += c.count;
        total_len += c.length;
    } while (total_count < nspec);
    auto chunk_json = [&](const Chunk& c, bool header) {
        std::string o = "{\"version\":\"1\",\"segmentCount\":" + std::to_string(c.count) + ",\"length\":" +
                        std::to_string(c.length) + ",\"segments\":[";
        for (uint32_t k = 0; k < c.count; k++) {
            if (k) o += ',';
            o += specs[c.start + k];
        }
        o += "],\"startIndex\":" + std::to_string(c.start);
        if (header) {
            o += ",\"headerMetadata\":{\"minSequenceNumber\":" + std::to_string(h.sc.min_seq) +
                 ",\"sequenceNumber\":" + std::to_string(h.sc.cur_seq) + ",\"orderedChunkMetadata\":[{\"id\":\"header\"}";
            for (size_t b = 1; b < chunks.size(); b++) o += ",{\"id\":\"body_" + std::to_string(b - 1) + "\"}";
            o += "],\"totalLength\":" + std::to_string(total_len) + ",\"totalSegmentCount\":" +
                 std::to_string(total_count) + '}';
        }
        return o + '}';
    };
    std::string o = "{\"header\":" + chunk_json(chunks[0], true);
    for (size_t b = 1; b < chunks.size(); b++) o += ",\"body_" + std::to_string(b - 1) + "\":" + chunk_json(chunks[b], false);
    return o + '}';
}

// Documents [d0, d0 + n) to the host in one pass: every field of the range in one copy each, the
// text arenas per document, all asynchronous behind one synchronisation
mt_status read_range(mt_engine* e, uint32_t d0, uint32_t n, std::vector<HostDoc>& out) {
    const mt_gstate& g = e->g;
    std::vector<mt_doc_scalars> sc(n);
    HIP_OK(hipMemcpyAsync(sc.data(), g.sc + d0, n * sizeof(mt_doc_scalars), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    const size_t S = (size_t)n * g.segcap, so = (size_t)d0 * g.segcap;
    std::vector<int32_t> seq, rseq;
    std::vector<uint32_t> len, toff;
    std::vector<uint64_t> ovl, props, ovx, ph, pxl, pxh, pxx;
    std::vector<uint8_t> client, rclient, flags, lb, ib;
    std::vector<uint16_t> chi;
    bool any_wide = false;
    for (uint32_t i = 0; i < n; i++) any_wide = any_wide || ((sc[i].wide & MT_WIDE_DOC) && g.ovx);
    HIP_OK(fetch(seq, g.seq, so, S, e->stream));
    HIP_OK(fetch(rseq, g.rseq, so, S, e->stream));
    HIP_OK(fetch(len, g.len, so, S, e->stream));
    HIP_OK(fetch(toff, g.toff, so, S, e->stream));
    HIP_OK(fetch(ovl, g.ovl, so, S, e->stream));
    HIP_OK(fetch(props, g.props, so, S, e->stream));
    if (any_wide) {
        HIP_OK(fetch(ovx, g.ovx, so * MT_OVX_WORDS, S * MT_OVX_WORDS, e->stream));
        HIP_OK(fetch(chi, g.chi, so, S, e->stream));
        HIP_OK(fetch(ph, g.ph, so, S, e->stream));
        HIP_OK(fetch(pxl, g.pxl, so, S, e->stream));
        HIP_OK(fetch(pxh, g.pxh, so, S, e->stream));
        HIP_OK(fetch(pxx, g.pxx, so * 4, S * 4, e->stream));
    }
    HIP_OK(fetch(client, g.client, so, S, e->stream));
    HIP_OK(fetch(rclient, g.rclient, so, S, e->stream));
    HIP_OK(fetch(flags, g.flags, so, S, e->stream));
    HIP_OK(fetch(lb, g.lbcnt, (size_t)d0 * g.lbcap, (size_t)n * g.lbcap, e->stream));
    HIP_OK(fetch(ib, g.ibcnt, (size_t)d0 * (MT_MAXLEV - 1) * g.ibcap, (size_t)n * (MT_MAXLEV - 1) * g.ibcap, e->stream));
    out.assign(n, HostDoc());
    HIP_OK(hipStreamSynchronize(e->stream));
    for (uint32_t i = 0; i < n; i++) {
        HostDoc& h = out[i];
        h.sc = sc[i];
        h.wide = (sc[i].wide & MT_WIDE_DOC) && g.ovx;
        mt_status st = fetch_text(e, d0 + i, sc[i], h.text);
        if (st) return st;
        const size_t a = (size_t)i * g.segcap, m = (size_t)h.sc.nseg;
        h.seq.assign(seq.begin() + a, seq.begin() + a + m);
        h.rseq.assign(rseq.begin() + a, rseq.begin() + a + m);
        h.len.assign(len.begin() + a, len.begin() + a + m);
        h.toff.assign(toff.begin() + a, toff.begin() + a + m);
        h.ovl.assign(ovl.begin() + a, ovl.begin() + a + m);
        h.props.assign(props.begin() + a, props.begin() + a + m);
        if (h.wide) {
            h.ovx.assign(ovx.begin() + a * MT_OVX_WORDS, ovx.begin() + (a + m) * MT_OVX_WORDS);
            h.chi.assign(chi.begin() + a, chi.begin() + a + m);
            h.ph.assign(ph.begin() + a, ph.begin() + a + m);
            h.pxl.assign(pxl.begin() + a, pxl.begin() + a + m);
            h.pxh.assign(pxh.begin() + a, pxh.begin() + a + m);
            h.pxx.assign(pxx.begin() + a * 4, pxx.begin() + (a + m) * 4);
        }
        h.client.assign(client.begin() + a, client.begin() + a + m);
        h.rclient.assign(rclient.begin() + a, rclient.begin() + a + m);
        h.flags.assign(flags.begin() + a, flags.begin() + a + m);
        h.levels.resize(h.sc.nlev);
        for (int L = 0; L < h.sc.nlev; L++) {
            const uint8_t* src = L == 0 ? lb.data() + (size_t)i * g.lbcap
                                        : ib.data() + ((size_t)i * (MT_MAXLEV - 1) + (L - 1)) * g.ibcap;
            h.levels[L].assign(src, src + h.sc.nb[L]);
        }
    }
    return MT_OK;
}

mt_status copy_out(const std::string& s, char* buf, uint64_t cap, uint64_t* len) {
    if (len) *len = s.size();
    if (buf && cap) {
        const uint64_t n = std::min<uint64_t>(cap - 1, s.size());
        memcpy(buf, s.data(), n);
        buf[n] = 0;
    }
    return MT_OK;
}
}  // namespace

extern "C" {

mt_status mt_get_state(mt_engine* e, uint32_t doc, char* buf, uint64_t cap, uint64_t* len) {
    if (!e || doc >= e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HostDoc h;
    mt_status st = read_doc(e, doc, h);
    if (st) return st;
    return copy_out(state_json(h), buf, cap, len);
}

mt_status mt_get_snapshot(mt_engine* e, uint32_t doc, uint32_t chunk_size, const char* const* client_names,
                          uint32_t n_names, char* buf, uint64_t cap, uint64_t* len) {
    if (!e || doc >= e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HostDoc h;
    mt_status st = read_doc(e, doc, h);
    if (st) return st;
    const uint32_t scap = std::max<uint32_t>(1, (uint32_t)h.sc.nseg);
    std::vector<uint32_t> sp(3 * (size_t)scap);
    uint32_t nspec = 0;
    mt_scratch s;
    auto [d_n, d_sp] = s.carve<uint32_t, uint32_t>(1, sp.size());
    st = mt_chain(e->stream, s.status())
             .launch(mt_launch_snapshot, &e->g, doc, 1, scap, d_sp, d_n, e->stream)
             .d2h(&nspec, d_n, sizeof nspec)
             .d2h(sp.data(), d_sp, sp.size() * sizeof(uint32_t))
             .sync().status();
    if (st) return st;
    if (nspec > scap) return MT_ERR_STATE;
    return copy_out(snapshot_json(h, sp, nspec, chunk_size ? chunk_size : 10000u, client_names, n_names), buf, cap,
                    len);
}

mt_status mt_get_snapshots(mt_engine* e, uint32_t d0, uint32_t n, uint32_t chunk_size, const char* const* client_names,
                           uint32_t n_names, char* buf, uint64_t cap, uint64_t* offsets) {
    if (!e || !offsets || d0 > e->n_docs || n > e->n_docs - d0) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    // a sizing call (buf NULL) leaves its result for the copying call with the same arguments
    auto& c = e->snap_cache;
    const bool hit = c.valid && c.gen == e->gen && c.d0 == d0 && c.n == n && c.chunk == chunk_size && c.names == client_names &&
                     c.n_names == n_names;
    if (!hit) {
        c.valid = false;
        c.json.clear();
        c.off.assign(n + 1, 0);
        if (n) {
            std::vector<HostDoc> docs;
            mt_status st = read_range(e, d0, n, docs);
            if (st) return st;
            // the device extraction of every document in one launch
            const uint32_t scap = e->g.segcap;
            std::vector<uint32_t> hc(n), hs((size_t)n * scap * 3);
            {
                mt_scratch s;
                auto [specs, counts] = s.carve<uint32_t, uint32_t>(hs.size(), n);
                st = mt_chain(e->stream, s.status())
                         .launch(mt_launch_snapshot, &e->g, d0, n, scap, specs, counts, e->stream)
                         .d2h(hc.data(), counts, n * sizeof(uint32_t))
                         .d2h(hs.data(), specs, hs.size() * sizeof(uint32_t))
                         .sync().status();
                if (st) return st;
            }
            // the JSON of each document on the host cores, in parallel
            std::vector<std::string> parts(n);
            std::atomic<uint32_t> next{0};
            std::atomic<int> bad{0};
            const unsigned nt = std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), std::min(16u, n));
            auto work = [&] {
                for (uint32_t i; (i = next.fetch_add(1)) < n;) {
                    if (hc[i] > scap) {
                        bad = 1;
                        continue;
                    }
                    std::vector<uint32_t> sp(hs.begin() + (size_t)i * scap * 3, hs.begin() + ((size_t)i * scap + hc[i]) * 3);
                    parts[i] = snapshot_json(docs[i], sp, hc[i], chunk_size ? chunk_size : 10000u, client_names, n_names);
                }
            };
            std::vector<std::thread> th;
            for (unsigned t = 1; t < nt; t++) th.emplace_back(work);
            work();
            for (auto& x : th) x.join();
            if (bad) return MT_ERR_STATE;
            for (uint32_t i = 0; i < n; i++) c.off[i + 1] = c.off[i] + parts[i].size();
            c.json.reserve(c.off[n]);
            for (auto& p : parts) c.json += p;
        }
        c.valid = true;
        c.gen = e->gen;
        c.d0 = d0;
        c.n = n;
        c.chunk = chunk_size;
        c.names = client_names;
        c.n_names = n_names;
    }
    for (uint32_t i = 0; i <= n; i++) offsets[i] = c.off[i];
    if (!buf) return MT_OK;
    if (cap < c.json.size()) return MT_ERR_ARG;
    memcpy(buf, c.json.data(), c.json.size());
    c.valid = false;  // consumed
    c.json.clear();
    c.json.shrink_to_fit();
    return MT_OK;
}

mt_status mt_snapshot_extract(mt_engine* e, uint32_t d0, uint32_t n, float* kernel_ms, uint64_t* n_specs) {
    if (!e || d0 > e->n_docs || n > e->n_docs - d0) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    if (n == 0) return MT_OK;
    const uint32_t cap = e->g.segcap;
    mt_scratch s;
    auto [specs, counts] = s.carve<uint32_t, uint32_t>((size_t)n * cap * 3, n);
    float ms = 0.f;
    std::vector<uint32_t> hc(n);
    const mt_status st = mt_chain(e->stream, s.status())
                             .launch(hipEventRecord, e->ev0, e->stream)  // (the events around the launch only)
                             .launch(mt_launch_snapshot, &e->g, d0, n, cap, specs, counts, e->stream)
                             .launch(hipEventRecord, e->ev1, e->stream)
                             .launch(hipEventSynchronize, e->ev1)
                             .launch(hipEventElapsedTime, &ms, e->ev0, e->ev1)
                             .launch(hipMemcpy, hc.data(), counts, n * sizeof(uint32_t), hipMemcpyDeviceToHost)
                             .status();
    if (st) return st;
    uint64_t tot = 0;
    for (uint32_t c : hc) tot += c;
    if (kernel_ms) *kernel_ms = ms;
    if (n_specs) *n_specs = tot;
    return MT_OK;
}

mt_status mt_get_text(mt_engine* e, uint32_t doc, char* buf, uint64_t cap, uint64_t* len) {
    if (!e || doc >= e->n_docs) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HostDoc h;
    mt_status st = read_doc(e, doc, h);
    if (st) return st;
    std::string t;  // UTF-16 code units, little endian
    for (int i = 0; i < h.sc.nseg; i++)
        if (!(h.flags[i] & (MT_SF_REMOVED | MT_SF_MARKER)))  // gatherText: text segments only
            for (uint32_t q = 0; q < h.len[i]; q++) {
                t += (char)(h.units(i)[q] & 0xFF);
                t += (char)(h.units(i)[q] >> 8);
            }
    return copy_out(t, buf, cap, len);
}

mt_status mt_get_length(mt_engine* e, uint32_t doc, uint32_t* len) {
    if (!e || doc >= e->n_docs || !len) return MT_ERR_ARG;
    HIP_OK(hipSetDevice(e->cfg.device));
    HostDoc h;
    mt_status st = read_doc(e, doc, h);
    if (st) return st;
    uint32_t n = 0;
    for (int i = 0; i < h.sc.nseg; i++)
        if (!(h.flags[i] & MT_SF_REMOVED)) n += h.len[i];
    *len = n;
    return MT_OK;
}

}  // extern "C"
