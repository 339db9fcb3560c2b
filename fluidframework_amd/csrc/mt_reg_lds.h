// mt_reg_lds.h -- the register engine's per-wave LDS block (mt_apply_reg.hip).  Plain C++: a host
// program can include it to print the sizes (tests/test_reg_lds_layout.py, tools/resource_usage.py).
#pragma once
#include <stdint.h>

#include <type_traits>

#include "mt_state.h"

namespace mtr {

constexpr int kMaxNodes = 8;           // MaxNodesInBlock, mergeTree.ts:334

template <int K>
struct RLds {
    static constexpr int CAP = 64 * K;
    // leaf blocks, blocks per interior level, heap entries (1-based): the class limits of mt::Lds at
    // CAP, and at least those of the 256 class -- the launch's worst-case growth (mt_bin_kernel: 2 leaf
    // blocks, 1 interior block and 4 heap entries per op) needs them for a b = 32 launch to fit the
    // 192 class at all (mt_engine.cpp kClassParams)
    static constexpr int LB = CAP / 2 > 128 ? CAP / 2 : 128;
    static constexpr int IB = CAP / 8 + 8 > 40 ? CAP / 8 + 8 : 40;
    static constexpr int H = CAP / 2 + 64 > 192 ? CAP / 2 + 64 : 192;
    // props: by segment id, 8 keys x u8 value id.  scr: the store's staging by position / leaf block.
    // tln: by segment id, the text length while linked, 0 once unlinked (the op loop's compaction; during
    // load: the leaf-block marks by position).
    // From K = 8 up (round 10) scr shares props' words -- the store reads every live segment's props into
    // registers first and stages through scr after -- and tln is 16 bits wide like toff and the arena: 6 B
    // per slot less LDS than the older form, where LDS admitted fewer waves than the registers.
    // The classes up to K = 7 have the LDS for every wave their registers admit and keep the older form
    // (SCR_OWN): 32-bit lengths that share their words with staging words of the class's own (neither is
    // live while the other is: load writes tln after its last read of the marks, store runs after the op
    // loop), and the store reads props where it writes them.  (C5's K = 2 / 3 documents, stored after every
    // 32 ops, lost 0.4 % with the new form.)
    static constexpr bool SCR_OWN = K <= 7;
    using tln_t = std::conditional_t<SCR_OWN, uint32_t, uint16_t>;
    union {
        uint64_t props[CAP];
        int32_t scr_props[CAP + 1];
    };
    union {
        int32_t scr_own[SCR_OWN ? CAP + 1 : 1];
        uint32_t tln32[SCR_OWN ? CAP + 1 : 1];
    };
    union {
        struct {
            // scour scratch: the live children by rank, one array per field (separate 4-byte stores: no
            // 4-register tuple built per slot, which cost ~20 VGPRs at the scour's register peak)
            // zr[q]: the removal seq of a removed child q, else its seq; zr[8 + q] its li, zr[16 + q] its
            // cf, zr[24 + q] its slot
            uint32_t zr[4 * kMaxNodes];
            // the lanes' discard words of the branch-free LDS stores (a lane with nothing to store
            // writes here; never read)
            uint64_t dum[64];
        };
        // store staging: needsScour per leaf block (written after the store's last discarded write)
        uint8_t lbsc[LB + 1];
    };
    int32_t hseq[H];
    int32_t nb[MT_MAXLEV];  // blocks per interior level (leaf blocks are counted by BS bits)
    // (16-bit tln) the id of the one segment whose text fills a 64 KiB arena half (its length is 0 in
    // tln's 16 bits), else -1: only compact_text tells the two apart
    int32_t big;
    uint16_t tln16[SCR_OWN ? 1 : CAP];
    uint16_t toff[CAP];     // by segment id: text view offset (at store: id -> position)
    uint16_t hslot[H];      // heap entry -> segment id
    uint8_t ibcnt[MT_MAXLEV - 1][IB];  // interior levels: level L's child counts in ibcnt[L - 1]
};
// LDS is allocated per wave in 512-byte granules of a CU's 160 KiB (the waves resident at K = 9 are
// measured).  K = 9 fits 16 waves per CU (four per SIMD, its register
// occupancy), K = 10 14, K = 11 13, K = 12 12; profiles/r10_resource_usage_reg.txt has every class
static_assert(sizeof(RLds<9>) <= 10240, "RLds<9>: 16 waves per CU");
static_assert(sizeof(RLds<10>) <= 11264, "RLds<10>: 14 waves per CU");
static_assert(sizeof(RLds<11>) <= 12288 && sizeof(RLds<12>) <= 13312, "RLds<11> / <12>: 13 / 12 waves per CU");
static_assert(sizeof(RLds<8>::scr_props) <= sizeof(RLds<8>::props) && RLds<2>::LB <= RLds<2>::CAP, "scr inside props");
static_assert(sizeof(RLds<16>::lbsc) <= sizeof(RLds<16>::zr) + sizeof(RLds<16>::dum), "lbsc inside zr + dum");

}  // namespace mtr
