// mt_view.h -- a leaf's length in a view: nodeLength's leaf branch (mergeTree.ts:1659-1697) over the
// compact state in HBM, shared by the read kernels (mt_resolve_kernel, mt_text_ranges_kernel).
#pragma once
#include "../../include/mtgpu.h"
#include "mt_checksum.h"
#include "mt_state.h"

// The view of a read: the local view (ref_seq == MT_POS_LOCAL: Client's own reads -- a removed segment
// has length 0, an editing client's pending inserts count and its pending removals hide), or what
// client C had seen at refSeq R.
struct mt_view {
    bool local;
    bool wdoc;   // a wide document (MT_WIDE_DOC)
    int form;    // mt_form of the document
    int32_t R;
    uint32_t C;
};

MT_HD static inline mt_view mt_view_of(const mt_doc_scalars& sc, int32_t ref_seq, uint32_t client) {
    const bool wdoc = (sc.wide & MT_WIDE_DOC) != 0;
    return mt_view{ref_seq == MT_POS_LOCAL, wdoc, mt_form(wdoc, sc.wide), ref_seq, client};
}

// the view length of the segment at HBM index i (= doc * segcap + ordinal)
MT_HD static inline int mt_view_len(const mt_gstate& g, const mt_view& v, size_t i) {
    const bool rm = (g.flags[i] & MT_SF_REMOVED) != 0;
    if (v.local) return rm ? 0 : (int)g.len[i];
    // (pending local edits: seq / removedSeq -1, UnassignedSequenceNumber, seen by no refSeq)
    const bool seen = mt_gclient(g, v.wdoc, i) == v.C || (g.seq[i] != -1 && g.seq[i] <= v.R);
    const bool ov = v.C < 64 ? ((g.ovl[i] >> v.C) & 1ull) != 0
                             : (v.wdoc && mt_ovx_has2(mt_govx_lo(g, i), mt_govx_hi(g, v.form, i), v.C));
    const bool hid = rm && (mt_grclient(g, v.wdoc, i) == v.C || ov || (g.rseq[i] != -1 && g.rseq[i] <= v.R));
    return (seen && !hid) ? (int)g.len[i] : 0;
}
