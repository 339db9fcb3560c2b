// mt_launch.h -- every launcher and helper that crosses a file of libmtgpu.so, declared once.
//
// The .hip files define these (extern "C": unmangled, so the names carry no types); the host files
// call them.  Both sides include this header, so a definition that disagrees with its declaration
// is a compile error ("conflicting types") instead of a call that links and passes garbage.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mtgpu.h"

struct mt_gstate;  // mt_state.h

extern "C" {

// ---- mt_apply.hip: the LDS engine, its forms, the generator
hipError_t mt_launch_apply(int cap_class, const mt_gstate* g, const mt_op_rec* ops, const uint8_t* payload,
                           const uint32_t* row_ptr, const uint32_t* doc_ids, uint32_t n_docs, uint32_t op_lo,
                           uint32_t op_cnt, hipStream_t stream);
hipError_t mt_launch_apply_loc(int cap_class, const mt_gstate* g, const mt_op_rec* ops, const uint8_t* payload,
                               const uint32_t* row_ptr, const uint32_t* doc_ids, uint32_t n_docs, uint32_t op_lo,
                               uint32_t op_cnt, hipStream_t stream);
hipError_t mt_launch_apply_big(int cap_class, const mt_gstate* g, const mt_op_rec* ops, const uint8_t* payload,
                               const uint32_t* row_ptr, const uint32_t* doc_ids, uint32_t n_docs, uint32_t op_lo,
                               uint32_t op_cnt, uint8_t* ws, hipStream_t stream);
hipError_t mt_launch_apply_wide(int cap_class, const mt_gstate* g, const mt_op_rec* ops, const uint8_t* payload,
                                const uint32_t* row_ptr, const uint32_t* doc_ids, uint32_t n_docs, uint32_t op_lo,
                                uint32_t op_cnt, uint8_t* ws, int xl, hipStream_t stream);
hipError_t mt_launch_apply_loc_big(int cap_class, int gw, const mt_gstate* g, const mt_op_rec* ops,
                                   const uint8_t* payload, const uint32_t* row_ptr, const uint32_t* doc_ids,
                                   uint32_t n_docs, uint32_t op_lo, uint32_t op_cnt, uint8_t* ws, hipStream_t stream);
// (the wide editing form: cap_class 1024 / 4096 / 8192, gw 1 or MT_LOC_GW; ws: n_docs * mt_lds_bytes_loc_wide)
hipError_t mt_launch_apply_loc_wide(int cap_class, int gw, const mt_gstate* g, const mt_op_rec* ops,
                                    const uint8_t* payload, const uint32_t* row_ptr, const uint32_t* doc_ids,
                                    uint32_t n_docs, uint32_t op_lo, uint32_t op_cnt, uint8_t* ws, hipStream_t stream);
hipError_t mt_launch_gen(int cap_class, const mt_gstate* g, const mt_synth_cfg* cfg, uint32_t doc_id_base,
                         const uint32_t* gids, int32_t* cref, int32_t* stall, uint32_t* pay_used, uint32_t paycap,
                         mt_op_rec* ops, uint8_t* payload, const uint32_t* row_ptr, const uint32_t* doc_ids,
                         uint32_t n_docs, uint32_t op_lo, uint32_t op_cnt, hipStream_t stream);
size_t mt_lds_bytes(int cap_class);
size_t mt_lds_bytes_wide(int cap_class);
size_t mt_lds_bytes_loc(int cap_class, int gw);
size_t mt_lds_bytes_loc_wide(int cap_class, int gw);

// ---- mt_apply_reg.hip: the register engine
hipError_t mt_launch_apply_reg(int cap_class, int form, const mt_gstate* g, const mt_op_rec* ops,
                               const uint8_t* payload, const uint32_t* row_ptr, const uint32_t* doc_ids,
                               uint32_t n_docs, uint32_t op_lo, uint32_t op_cnt, hipStream_t stream);

// ---- mt_service.hip: init / load, binning, fixup, queries, checksums, snapshot extraction
hipError_t mt_launch_init(const mt_gstate* g, uint32_t n_docs, hipStream_t st);
hipError_t mt_launch_label_keys(const mt_gstate* g, uint32_t d0, uint32_t d1, uint32_t keys, hipStream_t st);
hipError_t mt_launch_load(const mt_gstate* g, uint32_t n, const uint32_t* doc_ids, const uint32_t* row_ptr,
                          const mt_load_seg* segs, const uint8_t* text, const int32_t* min_seq,
                          const int32_t* cur_seq, hipStream_t st);
hipError_t mt_launch_bin(const mt_gstate* g, const uint32_t* row_ptr, uint32_t n_docs, uint32_t op_lo,
                         uint32_t op_cnt, const int32_t* classes, int n_classes, int first_lds, int first_wide,
                         uint32_t* counts, uint32_t* ids, const mt_op_rec* ops, const uint8_t* payload,
                         unsigned long long* acc, hipStream_t st);
hipError_t mt_launch_scan_records(const mt_op_rec* ops, uint64_t n_ops, uint64_t payload_bytes, uint32_t* flags,
                                  hipStream_t st);
hipError_t mt_launch_fixup(const mt_gstate* g, const mt_op_rec* ops, uint32_t n_docs, hipStream_t st);
hipError_t mt_launch_tiles(const mt_gstate* g, const mt_tile_query* q, uint32_t n, mt_tile_result* out,
                           hipStream_t st);
hipError_t mt_launch_stacks(const mt_gstate* g, const mt_tile_query* q, uint32_t n, uint32_t cap,
                            mt_stack_item* items, uint32_t* depth, hipStream_t st);
hipError_t mt_launch_resolve(const mt_gstate* g, const mt_pos_query* q, uint32_t n, uint32_t n_docs,
                             mt_pos_result* out, hipStream_t st);
hipError_t mt_launch_seginfo(const mt_gstate* g, const uint32_t* docs, const int32_t* ords, uint32_t n,
                             mt_seg_info* out, hipStream_t st);
hipError_t mt_launch_events_pack(const mt_gstate* g, uint32_t n_docs, const uint64_t* off, mt_event* out,
                                 hipStream_t st);
hipError_t mt_launch_checksum(const mt_gstate* g, uint32_t n_docs, uint64_t* out, hipStream_t st);
hipError_t mt_launch_snapshot(const mt_gstate* g, uint32_t d0, uint32_t n_docs, uint32_t cap, uint32_t* specs,
                              uint32_t* counts, hipStream_t st);

// ---- mt_refs.hip: local references
hipError_t mt_launch_refs_track(const mt_gstate* g, uint32_t n_docs, hipStream_t st);
hipError_t mt_launch_refs_claim(const mt_gstate* g, const mt_ref_add* in, const mt_pos_result* at, uint32_t n,
                                uint32_t n_docs, uint32_t* handles, hipStream_t st);
hipError_t mt_launch_refs_release(const mt_gstate* g, const uint32_t* docs, const uint32_t* handles, uint32_t n,
                                  uint32_t n_docs, hipStream_t st);
hipError_t mt_launch_refs_free_docs(const mt_gstate* g, const uint32_t* ids, uint32_t n, uint32_t n_docs,
                                    hipStream_t st);
hipError_t mt_launch_refs_resolve_docs(const mt_gstate* g, const uint32_t* docs, uint32_t n, uint32_t n_docs,
                                       hipStream_t st);
hipError_t mt_launch_refs_positions(const mt_gstate* g, const uint32_t* docs, const uint32_t* handles, uint32_t n,
                                    uint32_t n_docs, mt_ref_pos* out, hipStream_t st);
hipError_t mt_launch_refs_stamp(const mt_gstate* g, const uint32_t* docs, const mt_ref_pos* at, mt_op_rec* ops,
                                uint32_t n, uint32_t n_docs, int32_t* positions, hipStream_t st);

// ---- mt_intervals.hip: interval collections
hipError_t mt_launch_intervals_overlap(const mt_gstate* g, const mt_interval_query* q, uint32_t n, uint32_t n_docs,
                                       const uint32_t* row_ptr, uint32_t* counts, uint32_t* out, hipStream_t st);
hipError_t mt_launch_intervals_claim(const mt_gstate* g, const mt_interval_add* in, const mt_pos_result* at,
                                     uint32_t n, uint32_t n_docs, uint32_t* handles, hipStream_t st);
hipError_t mt_launch_intervals_release(const mt_gstate* g, const mt_interval_query* q, uint32_t n, uint32_t n_docs,
                                       uint32_t* removed, hipStream_t st);
hipError_t mt_launch_intervals_free_docs(const mt_gstate* g, const uint32_t* ids, uint32_t n, uint32_t n_docs,
                                         hipStream_t st);
hipError_t mt_launch_intervals_gather(const mt_gstate* g, const uint32_t* docs, uint32_t n, uint32_t n_docs,
                                      mt_interval_pos* out, hipStream_t st);

// ---- mt_ckpt.hip: document checkpoints (mt_ckpt.h)
// hdr[i] = the checkpoint header of document ids[i] (sizes follow from it: mt_ckpt_walk)
hipError_t mt_launch_ckpt_size(const mt_gstate* g, const uint32_t* ids, uint32_t n, struct mt_ckpt_dochdr* hdr,
                               hipStream_t st);
// document ids[i] packed at out + off[i] (hdr: the sizing launch's); parts: workgroups per document
hipError_t mt_launch_ckpt_pack(const mt_gstate* g, const uint32_t* ids, uint32_t n, const struct mt_ckpt_dochdr* hdr,
                               const uint64_t* off, uint8_t* out, uint32_t parts, hipStream_t st);
// the (checked) document at in + off[i] into slot ids[i]
hipError_t mt_launch_ckpt_unpack(const mt_gstate* g, const uint32_t* ids, uint32_t n, const uint64_t* off,
                                 const uint8_t* in, uint32_t parts, hipStream_t st);
// the editing clients' sections of the same documents (a launch of their own, after the one above, when a
// document of the call is an editing client's; n = 0: none is, nothing is launched)
hipError_t mt_launch_ckpt_pack_loc(const mt_gstate* g, const uint32_t* ids, uint32_t n, const struct mt_ckpt_dochdr* hdr,
                                   const uint64_t* off, uint8_t* out, uint32_t parts, hipStream_t st);
hipError_t mt_launch_ckpt_unpack_loc(const mt_gstate* g, const uint32_t* ids, uint32_t n, const uint64_t* off,
                                     const uint8_t* in, uint32_t parts, hipStream_t st);

// ---- mt_text.hip: text reads
hipError_t mt_launch_text_ranges(const mt_gstate* g, const mt_text_query* q, uint32_t n, uint32_t n_docs,
                                 const uint32_t* row_ptr, uint16_t* units, const uint32_t* m_row_ptr,
                                 mt_text_marker* markers, mt_text_count* counts, hipStream_t st);

// ---- mt_markers.hip: marker ids
hipError_t mt_launch_marker_positions(const mt_gstate* g, const mt_marker_query* q, uint32_t n, uint32_t n_docs,
                                      mt_marker_result* out, hipStream_t st);

// ---- mt_deli.hip: the ticket kernel on the apply engine's stream (mt_submit_ticks_deli)
mt_status mt_deli_ticket_on_stream(mt_deli* dl, int32_t device, hipStream_t st, const mt_raw_msg* d_msgs,
                                   const uint32_t* d_row_ptr, uint32_t n_docs, mt_ticket* d_out, mt_op_rec* d_ops,
                                   uint64_t n_ops);

}  // extern "C"
