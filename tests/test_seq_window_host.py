"""csrc/mt_seqwin.h on the host: the register engine's window offsets (pack, compare, unpack)
against plain 32-bit compares, over the edge values of the encoding and bases next to 0 and to
INT32_MAX.  The header is plain C; the host compiler builds it into a small program."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#include "mt_seqwin.h"

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fails++; printf("line %d: %s (B=%d v=%d r=%d R=%d)\n", __LINE__, #c, B, v, r, R); } } while (0)

int main(void) {
    const int32_t top = 0x7fffffff;
    const int32_t bases[] = {0, 1, 7, 1000000, top - 0x7FFF, top - 0x7FFE, top - 1, top};
    const uint32_t offs[] = {0u, 1u, 2u, 0x3FFFu, 0x7FFDu, MT_SW_MAX};
    const int32_t under[] = {0, 1, 5, 0x7FFF, 0x10000};          /* how far at or below B a value lies */
    const uint32_t lims[] = {0u, 1u, 2u, 0x7FFDu, MT_SW_MAX, 0x7FFFu, 0x12345u};  /* R - B */
    long n = 0;
    for (unsigned bi = 0; bi < sizeof bases / sizeof *bases; bi++) {
        const int32_t B = bases[bi];
        /* the values a document can hold: at or below B, and B + 1 .. B + MT_SW_MAX */
        int32_t vals[16];
        unsigned nv = 0;
        for (unsigned i = 0; i < sizeof under / sizeof *under; i++)
            if ((int64_t)B - under[i] >= 0) vals[nv++] = B - under[i];
        for (unsigned i = 1; i < sizeof offs / sizeof *offs; i++)
            if ((int64_t)B + offs[i] <= top) vals[nv++] = (int32_t)(B + offs[i]);
        for (unsigned vi = 0; vi < nv; vi++)
            for (unsigned ri = 0; ri < nv; ri++) {
                const int32_t v = vals[vi], r = vals[ri];
                const uint32_t w = mt_sw_pack(mt_sw_off(v, B), mt_sw_off(r, B));
                int32_t R = B;
                CHECK(mt_sw_dseq(w) == mt_sw_off(v, B) && mt_sw_drseq(w) == mt_sw_off(r, B));
                CHECK(mt_sw_dseq(w) <= MT_SW_MAX && mt_sw_drseq(w) <= MT_SW_MAX);
                CHECK((mt_sw_dseq(w) == 0) == (v <= B));
                /* unpack: exact above B, the row's own number at or below it */
                CHECK(mt_sw_exact(mt_sw_dseq(w), B, v) == v && mt_sw_exact(mt_sw_drseq(w), B, r) == r);
                if (v > B) CHECK(mt_sw_exact(mt_sw_dseq(w), B, -12345) == v);
                for (unsigned li = 0; li < sizeof lims / sizeof *lims; li++) {
                    if ((int64_t)B + lims[li] > top) continue;
                    R = (int32_t)(B + lims[li]);
                    const uint32_t lim = mt_sw_lim(R, B);
                    CHECK(lim <= MT_SW_MAX);
                    CHECK((mt_sw_seq_le(w, lim) != 0) == (v <= R));
                    CHECK((mt_sw_rseq_le(w, lim) != 0) == (r <= R));
                    /* a padding slot (seq INT32_MAX at the engines that keep 32 bits) is above every R
                       that an op can carry (R < S <= INT32_MAX) */
                    if (R < top) CHECK(!mt_sw_seq_le(mt_sw_pack(MT_SW_PAD, 0u), lim));
                    /* removedSeq == S for the S of the window, and the mark a remove leaves */
                    if (lims[li] >= 1u && lims[li] <= MT_SW_MAX) {
                        const int32_t S = R;
                        CHECK((mt_sw_rseq_eq(w, mt_sw_off(S, B)) != 0) == (r == S));
                        const uint32_t m = mt_sw_with_drseq(w, mt_sw_off(S, B));
                        CHECK(mt_sw_dseq(m) == mt_sw_dseq(w) && mt_sw_exact(mt_sw_drseq(m), B, 0) == S);
                    }
                    n++;
                }
            }
        /* the routing predicate: the last seq at most MT_SW_MAX above B, no reference below B */
        {
            int32_t v = 0, r = 0, R = 0;
            CHECK(mt_sw_fits(B, B, B));
            if ((int64_t)B + MT_SW_MAX <= top) CHECK(mt_sw_fits((int32_t)(B + MT_SW_MAX), B, B));
            if ((int64_t)B + MT_SW_MAX + 1 <= top) CHECK(!mt_sw_fits((int32_t)(B + MT_SW_MAX + 1), B, B));
            if (B < top) CHECK(mt_sw_fits(B, B + 1, B));
            if (B > 0) CHECK(!mt_sw_fits(B, B - 1, B) && !mt_sw_fits(B, 0, B) && mt_sw_fits(B - 1, B, B));
            CHECK(mt_sw_fits(B, top, B));
            if (B < top - 0x10000) CHECK(!mt_sw_fits(top, B, B));
        }
    }
    printf("%ld compares, %d failures\n", n, fails);
    return fails ? 1 : 0;
}
'''


def test_seq_window_helpers_on_the_host(tmp_path):
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
    if cc is None:
        pytest.fail('no host C compiler')
    src = tmp_path / 'seqwin.c'
    src.write_text(PROGRAM)
    exe = tmp_path / 'seqwin'
    subprocess.run([cc, '-O1', '-Wall', '-Werror', '-I', os.path.join(REPO, 'fluidframework_amd', 'csrc'),
                    '-o', str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:]
    assert int(r.stdout.split()[0]) > 1000
