/* mt_seqwin.h -- sequence numbers as offsets into the collab window.
 *
 * The register engine (mt_apply_reg.hip) keeps a segment's seq and removedSeq in one register for a
 * launch, as offsets from B, the document's minimum sequence number when the launch loaded it:
 *
 *     0            the value is at or below B (every view of the launch has seen it; the exact
 *                  number stays in the document's HBM row and is read back when the launch stores)
 *     1 .. 0x7FFE  value - B
 *     0x7FFF       a padding slot's seq (it compares above every reference sequence number)
 *
 * seq's offset is the word's high half, removedSeq's the low half (meaningful on a removed segment
 * only).  The compares of the op path -- seq <= R, removedSeq <= R, seq <= minSeq, removedSeq == S --
 * become compares of offsets; they are exact iff every R of the launch is >= B and every S of the
 * launch is at most B + 0x7FFE (mt_sw_fits; mt_bin_kernel sends a document whose launch does not fit
 * to the LDS engine, which keeps 32-bit numbers).
 * Plain C: the host compiler builds the same functions for tests/test_seq_window_host.py. */
#ifndef MT_SEQWIN_H
#define MT_SEQWIN_H
#include <stdint.h>

#ifndef MT_HD
#if defined(__HIPCC__)
#define MT_HD __host__ __device__
#else
#define MT_HD
#endif
#endif

#define MT_SW_MAX 0x7FFEu /* the largest offset of a value */
#define MT_SW_PAD 0x7FFFu /* a padding slot's seq */
/* The register classes up to K = MT_SW_EXACT_K (64 K slots) keep exact 32-bit numbers in two
 * registers: their launches need no window (mt_bin_kernel) */
#define MT_SW_EXACT_K 3

/* v as an offset from B (v <= B + MT_SW_MAX) */
MT_HD static inline uint32_t mt_sw_off(int32_t v, int32_t B) { return v <= B ? 0u : (uint32_t)v - (uint32_t)B; }
/* whether a launch whose largest sequence number is s_last, and whose smallest reference sequence
 * number is r_min, can run on offsets from B */
MT_HD static inline int mt_sw_fits(int32_t s_last, int32_t r_min, int32_t B) {
    return r_min >= B && (s_last <= B || (uint32_t)s_last - (uint32_t)B <= MT_SW_MAX);
}
MT_HD static inline uint32_t mt_sw_pack(uint32_t dseq, uint32_t drseq) { return (dseq << 16) | drseq; }
MT_HD static inline uint32_t mt_sw_dseq(uint32_t w) { return w >> 16; }
MT_HD static inline uint32_t mt_sw_drseq(uint32_t w) { return w & 0xFFFFu; }
MT_HD static inline uint32_t mt_sw_with_drseq(uint32_t w, uint32_t drseq) { return (w & 0xFFFF0000u) | drseq; }
/* a reference (or minimum) sequence number R >= B as the limit of the offset compares: every value's
 * offset is <= MT_SW_MAX, so a larger R - B compares the same */
MT_HD static inline uint32_t mt_sw_lim(int32_t R, int32_t B) {
    const uint32_t d = (uint32_t)R - (uint32_t)B;
    return d < MT_SW_MAX ? d : MT_SW_MAX;
}
/* seq <= R, removedSeq <= R, removedSeq == S with lim = mt_sw_lim(R, B), ds = mt_sw_off(S, B) */
MT_HD static inline int mt_sw_seq_le(uint32_t w, uint32_t lim) { return w < ((lim + 1u) << 16); }
MT_HD static inline int mt_sw_rseq_le(uint32_t w, uint32_t lim) { return mt_sw_drseq(w) <= lim; }
MT_HD static inline int mt_sw_rseq_eq(uint32_t w, uint32_t ds) { return mt_sw_drseq(w) == ds; }
/* the exact value of an offset d; at_load: the value the segment's origin row held when loaded */
MT_HD static inline int32_t mt_sw_exact(uint32_t d, int32_t B, int32_t at_load) {
    return d ? (int32_t)((uint32_t)B + d) : at_load;
}
#endif
