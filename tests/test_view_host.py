"""csrc/mt_view.h on the host: mt_view_of / mt_view_len over an mt_gstate filled with the rows of H0a
(32 overlapping removers >= 64 on one range: both halves of the list, ids >= 256 through chi),
wide_xl[0] (twenty of them), and wide_many[0] (ids >= 256) and H2c's first state (sixteen: the lo words
full) with form bit 4 clear and their hi words full of 0xFFFE, the id of the plan's stranger: a reader that
looks at words the document has not stored answers from garbage), for every
(segment, view) pair of the plan of tests/view_docs.py, against the plain rule there -- exactly.  The
headers build as they stand with the host compiler; the program is built plain and again with the
address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

import view_docs as vd

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'fluidframework_amd', 'csrc')

MT_WIDE_LDS, MT_WIDE_DOC, MT_WIDE_XOV = 1, 2, 128
MT_SF_REMOVED, MT_SF_MARKER = 1, 16
POS_LOCAL = -2**31

PROGRAM = r'''
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "mt_view.h"

// input: n_docs segcap; per document: nseg wide, then nseg rows
//   seq rseq len flags client rclient chi ovl ovx[0..7]
// then n_views and per view: doc ref_seq client.  Output: one line of view lengths per view.
int main(int argc, char** argv) {
    FILE* f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) return 2;
    unsigned n_docs, segcap;
    if (fscanf(f, "%u %u", &n_docs, &segcap) != 2) return 2;
    const size_t n = (size_t)n_docs * segcap;
    std::vector<int32_t> seq(n), rseq(n);
    std::vector<uint32_t> len(n);
    std::vector<uint8_t> flags(n), client(n), rclient(n);
    std::vector<uint64_t> ovl(n), ovx(n * MT_OVX_WORDS);
    std::vector<uint16_t> chi(n);
    std::vector<mt_doc_scalars> sc(n_docs);
    for (unsigned d = 0; d < n_docs; d++) {
        unsigned wide;
        sc[d] = mt_doc_scalars{};
        if (fscanf(f, "%d %u", &sc[d].nseg, &wide) != 2 || sc[d].nseg < 0 || (unsigned)sc[d].nseg > segcap) return 2;
        sc[d].wide = wide;
        for (int i = 0; i < sc[d].nseg; i++) {
            const size_t k = (size_t)d * segcap + i;
            unsigned fl, cl, rcl, hi;
            unsigned long long o, x[MT_OVX_WORDS];
            if (fscanf(f, "%d %d %u %u %u %u %u %llx %llx %llx %llx %llx %llx %llx %llx %llx", &seq[k], &rseq[k], &len[k],
                       &fl, &cl, &rcl, &hi, &o, &x[0], &x[1], &x[2], &x[3], &x[4], &x[5], &x[6], &x[7]) != 16)
                return 2;
            flags[k] = (uint8_t)fl, client[k] = (uint8_t)cl, rclient[k] = (uint8_t)rcl, chi[k] = (uint16_t)hi;
            ovl[k] = o;
            for (int q = 0; q < MT_OVX_WORDS; q++) ovx[k * MT_OVX_WORDS + q] = x[q];
        }
    }
    mt_gstate g{};
    g.seq = seq.data(), g.rseq = rseq.data(), g.len = len.data(), g.flags = flags.data();
    g.client = client.data(), g.rclient = rclient.data(), g.ovl = ovl.data(), g.ovx = ovx.data();
    g.chi = chi.data(), g.sc = sc.data(), g.segcap = segcap;
    unsigned n_views;
    if (fscanf(f, "%u", &n_views) != 1) return 2;
    for (unsigned v = 0; v < n_views; v++) {
        unsigned d, c;
        int r;
        if (fscanf(f, "%u %d %u", &d, &r, &c) != 3 || d >= n_docs) return 2;
        const mt_view view = mt_view_of(sc[d], r, c);
        for (int i = 0; i < sc[d].nseg; i++) printf("%d ", mt_view_len(g, view, (size_t)d * segcap + i));
        printf("\n");
    }
    fclose(f);
    return 0;
}
'''


def rows(state, hi_valid):
    """a canonical state as mt_state.h lays it out at rest: (nseg, wide bits, rows)"""
    out = []
    for text, seq, cl, rseq, rcl, ovl, _ in state['segs']:
        removed = rcl != -1
        hm = vd.high_members(ovl)
        assert len(hm) <= (32 if hi_valid else 16) and 0 < cl < 65535
        ids = hm + [0] * (32 - len(hm))
        words = [sum(ids[4 * w + q] << (16 * q) for q in range(4)) for w in range(8)]
        if not hi_valid:
            words[4:] = [0xFFFEFFFEFFFEFFFE] * 4   # 65534 sixteen times
        rc = rcl if removed else 0
        out.append([seq, rseq if removed else -1, vd.units(text),
                    (MT_SF_REMOVED if removed else 0) | (MT_SF_MARKER if isinstance(text, dict) else 0),
                    cl & 0xFF, rc & 0xFF, (cl >> 8) | ((rc >> 8) << 8), sum(1 << m for m in ovl if m < 64)] + words)
    return len(out), MT_WIDE_LDS | MT_WIDE_DOC | (MT_WIDE_XOV if hi_valid else 0), out


def documents(oracle):
    """[(label, state, form bit 4)]"""
    s = vd.Suite(oracle)
    pick = {'h0': True, 'wide_xl[0]': True, 'wide_many[0]': False, 'h2c': False}
    return [(lb, s.states[0][s.labels.index(lb)], hi) for lb, hi in pick.items()]


def write_input(path, docs, plans):
    laid = [rows(st, hi) for _, st, hi in docs]
    with open(path, 'w') as f:
        f.write('%d %d\n' % (len(docs), max(n for n, _, _ in laid)))
        for n, wide, rs in laid:
            f.write('%d %d\n' % (n, wide))
            for r in rs:
                f.write(' '.join(str(x) for x in r[:7]) + ' ' + ' '.join('%x' % x for x in r[7:]) + '\n')
        views = [(d, POS_LOCAL if r is None else r, c) for d, p in enumerate(plans) for r, c in p]
        f.write('%d\n' % len(views))
        for v in views:
            f.write('%d %d %d\n' % v)


def build(tmp_path, name, extra):
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    if cxx is None:
        pytest.fail('no host C++ compiler')
    src = tmp_path / 'view_host.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / name
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I', CSRC, *extra, '-o', str(exe), str(src)],
                   check=True)
    return exe


@pytest.mark.parametrize('sanitize', [False, True])
def test_view_len_on_the_host(tmp_path, oracle_lib, sanitize):
    docs = documents(oracle_lib)
    plans = [vd.plan(st) for _, st, _ in docs]
    # the three documents between them: both halves of the list, chi, and unstored hi words
    assert any(len(vd.high_members(s[5])) > 16 for s in docs[0][1]['segs'])
    assert any(max(s[5], default=0) >= 256 and s[4] >= 256 for s in docs[2][1]['segs'])
    assert any(len(vd.high_members(s[5])) == 16 for s in docs[3][1]['segs'])
    assert all((65534 in [c for _, c in p]) for p in plans)
    inp = tmp_path / 'rows.txt'
    write_input(inp, docs, plans)
    exe = build(tmp_path, 'view_host_san' if sanitize else 'view_host',
                ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'] if sanitize else [])
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-3000:])
    lines = r.stdout.strip().split('\n')
    k = pairs = 0
    bad = []
    for (label, st, _), p in zip(docs, plans):
        aliases = set(vd.alias_ids(st))
        for ref_seq, client in p:
            got = [int(x) for x in lines[k].split()]
            k += 1
            want = [vd.view_len(s, ref_seq, client) for s in st['segs']]
            pairs += len(want)
            if got != want:
                miss = [i for i in range(len(want)) if got[i] != want[i]]
                hit = sorted({c for i in miss for c in vd.classes(st['segs'][i], ref_seq, client, aliases)})
                bad.append((label, ref_seq, client, miss[0], got[miss[0]], want[miss[0]], hit))
    assert k == len(lines)
    assert not bad, '%d views differ, the first: %s; classes hit: %s' % (
        len(bad), bad[0], sorted({c for b in bad for c in b[6]}))
    assert pairs > 50000
