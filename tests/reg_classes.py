"""Helpers of test_reg_classes.py / test_reg_classes_gpu.py: steering a small document into any of the
register engine's 15 capacity classes (K = 2 ... 16, CAP = 64 K) by the size of its launch.

mt_bin_kernel (csrc/mt_service.hip) bins a document by the worst-case growth of its launch: a launch of
n records fits class {cap, lb, ib, h} (mt_engine.cpp kClassParams) when

    nseg + 2 n + n_empty + 1 <= cap        nb[0] + 2 n + 1 <= lb
    ib_need + n + 1 <= ib                  heap_n + 4 n + 16 <= h

with cap = 64 K, lb = max(cap / 2, 128), ib = max(cap / 8 + 8, 40), h = max(cap / 2 + 64, 192).  From
K = 5 up ib(K - 1) = 8 K, so a launch of exactly 8 K records cannot fit class K - 1 and fits class K as
long as the document is small (ib_need <= 7, heap_n <= 48, nb[0] <= 16 K - 1, nseg <= 48 K - 2 - n_empty).
The classes 128 / 192 / 256 share ib = 40 and h = 192: at n = 32 the segment count separates them
(nseg <= 62, 126, 190).  A log is brought to a launch size with non-op records (MT_OP_NOOP), which move
nothing but the document's current sequence number.

Not collected (no test_ prefix); every builder is cached and its results are shared, never changed."""
import functools

import numpy as np

INSERT, REMOVE, ANNOTATE, NOOP = 0, 1, 2, 3
MT_DERR_TEXT_ARENA = 5
ARENA = 64 * 1024

CLASS_FLAGS = 0xFC000000
MT_CLASS_EDITING, MT_CLASS_LDS, MT_CLASS_C64, MT_CLASS_WIDE = 0x40000000, 0x20000000, 0x10000000, 0x04000000
REG_MAX_CAP = 1024       # the classes above run on the LDS engine (mt_engine.cpp kRegMaxCap)
MT_SW_MAX, MT_SW_EXACT_K = 0x7FFE, 3   # csrc/mt_seqwin.h: the offset window of the classes above K = 3

K_ALL = tuple(range(2, 17))
K_ARENA = (7, 8, 9, 12, 16)   # 7: the last class of the older LDS block, 8: the first of the new, 9: four waves
K_HALT = (2, 7, 8, 9, 16)
FORMS = ('plain', 'c64', 'ev')
C64_SHIFT = 32           # hand-made logs: clients 1, 2, ... act as 33, 34, ... (ids past 32: the C64 form)
C64_CLIENTS = 48         # generated logs


def class_params(K):
    """{cap, lb, ib, h} of class K (mt_engine.cpp kClassParams, csrc/mt_reg_lds.h RLds<K>)"""
    cap = 64 * K
    return cap, max(cap // 2, 128), max(cap // 8 + 8, 40), max(cap // 2 + 64, 192)


def class_for(nseg, nb0, ib_need, heap_n, n_empty, n):
    """K of the smallest register class a launch of n records fits (None: past the 1024 class)"""
    for K in K_ALL:
        cap, lb, ib, h = class_params(K)
        if nseg + 2 * n + n_empty + 1 <= cap and nb0 + 2 * n + 1 <= lb and ib_need + n + 1 <= ib and \
                heap_n + 4 * n + 16 <= h:
            return K
    return None


FRESH = (0, 1, 0, 0, 1)  # (nseg, nb0, ib_need, heap_n, n_empty) of a new document: one empty leaf block


def launch_size(K):
    """records per launch that take a small document to class K: 8 K from K = 5 up; the three classes
    below share their block and heap limits, so at 32 the segment count decides among them"""
    if K not in K_ALL:
        raise ValueError('no register class K = %r' % (K,))
    return 32 if K <= 4 else 8 * K


def doc_shape(o, d):
    """(nseg, nb0, ib_need, heap_n, n_empty) of an oracle document, as mt_bin_kernel reads them from the
    stored state (the oracle's heap stands for the device's)"""
    st = o.state(d)
    tree = st['tree']  # child counts per level, the root's first, the leaf blocks' last
    return (len(st['segs']), len(tree[-1]), max([len(lv) for lv in tree[:-1]] or [0]), o.heap_size(d),
            sum(1 for c in tree[-1] if c == 0))


def fits_window(ops, min_seq, cur_seq):
    """mt_sw_fits for a launch's records: the classes above K = 3 keep sequence numbers as offsets from
    the document's min_seq; a launch outside runs on the LDS engine"""
    s_hi = max([cur_seq] + [int(s) for s in ops['seq']])
    refs = [int(r) for r, t in zip(ops['ref_seq'], ops['type']) if (int(t) & 7) != NOOP]
    return (not refs or min(refs) >= min_seq) and (s_hi <= min_seq or s_hi - min_seq <= MT_SW_MAX)


def _noops(last, count, same_seq):
    from fluidframework_amd.oplog import OP_DTYPE
    pad = np.zeros(count, dtype=OP_DTYPE)
    seq = int(last['seq'])
    pad['seq'] = seq if same_seq else np.arange(seq + 1, seq + 1 + count)
    pad['ref_seq'] = pad['seq'] - 1
    pad['msn'] = last['msn']
    pad['client'] = last['client']
    pad['type'] = NOOP
    return pad


def pad_launches(batch, real, n, same_seq=True):
    """Every `real` records of a document (a launch's share) followed by non-op records up to n records:
    the log replayed at ops_per_launch = n applies `real` of its records per launch.  The added records
    repeat the sequence number before them (a non-op message at the current sequence number is accepted
    and moves nothing at all), its msn and its client."""
    from fluidframework_amd.oplog import OpBatch
    assert 0 < real <= n
    out, rows = [], [0]
    for d in range(batch.n_docs):
        ops = batch.ops[int(batch.row_ptr[d]):int(batch.row_ptr[d + 1])]
        if not len(ops):
            raise ValueError('document %d has no record to pad after' % d)
        for a in range(0, len(ops), real):
            part = ops[a:a + real]
            out += [part, _noops(part[-1], n - len(part), same_seq)]
        rows.append(sum(len(x) for x in out))
    return OpBatch(np.concatenate(out), batch.payload, np.array(rows, dtype=np.uint32))


def pad_tail(batch, n):
    """MT_OP_NOOP records appended to every document until its row holds exactly n records: seq
    continuing from the document's last, ref_seq = seq - 1, the document's last msn, the last record's
    client.  A document of more than n records (or of none) is a mistake of the test's inputs."""
    counts = np.diff(batch.row_ptr.astype(np.int64))
    if len(counts) and (counts.max() > n or counts.min() < 1):
        raise ValueError('rows of %d ... %d records cannot be padded to %d' % (counts.min(), counts.max(), n))
    return pad_launches(batch, n, n, same_seq=False)


def launched(eng):
    """[(flags, capacity)] of the buckets that launched in the engine's last apply"""
    return [(cap & CLASS_FLAGS, cap & ~CLASS_FLAGS) for cap, _, launches, _ in eng.last_class_stats() if launches]


def no_lds_launches(eng):
    """nothing of the last apply ran on the LDS engine: no MT_CLASS_LDS / editing / wide bucket, and no
    class above the register engine's largest"""
    return all(not fl & (MT_CLASS_LDS | MT_CLASS_EDITING | MT_CLASS_WIDE) and cap <= REG_MAX_CAP
               for fl, cap in launched(eng))


def used_classes(eng, form):
    """{K} of the register classes that launched in the form's kernels in the last apply.  plain / ev:
    every bucket must be a plain one (the ev kernels report plain capacities; class_kernel names them);
    c64: the MT_CLASS_C64 buckets (a document joins them at its first record by a client past 32, so
    plain buckets may have launched before)."""
    got = launched(eng)
    want = MT_CLASS_C64 if form == 'c64' else 0
    assert all(fl in (0, want) for fl, _ in got), got
    ks = {cap // 64 for fl, cap in got if fl == want and cap <= REG_MAX_CAP}
    for K in ks:
        kernel = {'plain': 'mtr::reg_apply_kernel<%d>', 'c64': 'mtr::reg_apply_kernel_c64<%d>',
                  'ev': 'mtr::reg_apply_kernel_ev<%d>'}[form] % K
        assert eng.class_kernel(want | 64 * K) == kernel, (eng.class_kernel(want | 64 * K), kernel)
    return ks


def inserted_bytes(batch, d):
    a, b = int(batch.row_ptr[d]), int(batch.row_ptr[d + 1])
    ops = batch.ops[a:b]
    return int(ops['payload_len'][(ops['type'] & 7) == INSERT].sum())


def linked_text(o, d):
    """characters of every segment still in the tree, tombstones included, a marker counting 1: what a
    compaction of the text arena keeps"""
    return sum(len(s[0]) if isinstance(s[0], str) else 1 for s in o.state(d)['segs'])


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- A. documents around a segment that fills the whole 64 KiB arena half -------------------------
WHOLE = ''.join(chr(97 + (i * 7 + i // 26) % 26) for i in range(ARENA))  # no two windows of it alike nearby
FILL_A = ''.join(chr(65 + (i * 5 + i // 26) % 26) for i in range(40000))
FILL_B = ''.join(chr(48 + (i * 3 + i // 10) % 10) for i in range(40000))

# A scenario is a list of applies, each a list of (client, type, pos1, pos2, text, props[, 1]): the records
# take consecutive sequence numbers, ref_seq = msn = seq - 1 (every client has seen everything, so each
# message moves the collab window up to the one before it); with the trailing 1, msn = seq - 2.
_CUTS = [(2, REMOVE, 1000, 2000, None, None),
         (1, REMOVE, 0, 1, None, None),
         # (the msn reaches the second remove's seq before the insert: both tombstones are unlinked, so the
         # compaction that the insert needs frees their text.  Every acked piece next to another is longer
         # than TextSegmentGranularity, so zamboni appends none: an append's copy would need arena room
         # of its own)
         (2, REMOVE, 3000, 3001, None, None),
         (2, INSERT, 5, 0, 'y' * 50, {1: 3}),
         (1, INSERT, 60000, 0, 'zz\n', None)]
SCENARIOS = {
    # the two-record halt: the insert in front of the whole-arena segment has no room even after the
    # compaction (which moves the segment whole): MT_DERR_TEXT_ARENA at seq 2, the text intact
    'A1': [[(1, INSERT, 0, 0, WHOLE, None), (2, INSERT, 0, 0, 'x', None)]],
    # the segment cut by removes, its pieces unlinked, then an insert that fits only after a compaction
    'A2': [[(1, INSERT, 0, 0, WHOLE, None)] + _CUTS],
    # the segment removed whole and unlinked by a non-op message that moves the msn past the removal --
    # before the next insert, which needs a compaction (nothing is alive: it must copy nothing); that
    # insert removed and unlinked the same way, then a second client's insert that needs another one.
    # (The removes leave the msn below the insert they remove: the insert's LRU entry is still queued
    # when the non-op message moves the msn past both, and its scour finds the tombstone.  Had the msn
    # followed, that entry's scour would have come before the segment could go, and the remove's own
    # entry finds a block that needs no scour.)
    'A3': [[(1, INSERT, 0, 0, WHOLE, None), (2, REMOVE, 0, ARENA, None, None, 1), (1, NOOP, 0, 0, None, None),
            (1, INSERT, 0, 0, FILL_A, None), (2, REMOVE, 0, 40000, None, None, 1), (1, NOOP, 0, 0, None, None),
            (2, INSERT, 0, 0, FILL_B, None), (1, INSERT, 100, 0, 'q\n', None)]],
    # A2 in two applies: the whole-arena segment is stored, then loaded before it is cut
    'A4': [[(1, INSERT, 0, 0, WHOLE, None)], list(_CUTS)],
    # 65535 characters (the largest length 16 bits hold as itself) and a 1-character segment of another
    # client (its props keep zamboni from appending it): the arena half is full, no segment is "big"
    'A5': [[(1, INSERT, 0, 0, WHOLE[:ARENA - 1], None), (2, INSERT, ARENA - 1, 0, '!', {2: 1})] + _CUTS],
}


def scenario_batches(name, n=None, shift=0):
    """The scenario's applies as one-document OpBatches, each padded to n records (None: as it is)."""
    from fluidframework_amd.oplog import build_batch
    out, seq = [], 0
    for part in SCENARIOS[name]:
        recs = []
        for client, typ, p1, p2, text, props, *lag in part:
            seq += 1
            recs.append((seq, seq - 1, seq - 1 - sum(lag), client + shift, typ, p1, p2, text, props, 0))
        b = build_batch([recs])
        if n is not None:
            b = pad_tail(b, n)
            seq = int(b.ops['seq'][-1])
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def scenario(name, n=None, shift=0):
    """(batches, oracle): the oracle (events recorded) after the scenario's applies.  A1's oracle stops
    before the record the engine halts on: the oracle has no arena to run out of."""
    batches = scenario_batches(name, n, shift)
    o = _oracle().Oracle(1).record_events()
    for b in batches:
        o.apply(b.split_ops(1)[0] if name == 'A1' else b)
    assert o.error(0) == (0, 0), (name, o.error(0))
    return batches, o


# ---- B. small generated documents in every class ---------------------------------------------------
N_DOCS = 8
WORKLOADS = {
    # test_gpu_engines.py's, with a collab window of at most 8 (the heap stays small)
    # removes outpace inserts: documents repeatedly shrink towards empty
    'shrink': dict(n_clients=8, max_lag=8, p_insert=0.3, p_remove=0.7),
    # annotate-heavy: property runs block zamboni appends
    'annotate': dict(n_clients=16, max_lag=8, n_keys=8, n_values=4, p_insert=0.4, p_remove=0.15, p_overlap=0.3,
                     p_null=0.2, p_rewrite=0.1, p_insert_props=0.3),
    # test_gpu_compaction.py's
    'churn': dict(n_clients=32, max_lag=8, n_keys=8, n_values=16, p_insert=0.5, p_remove=0.48, p_overlap=0.5,
                  p_insert_props=0.1),
}
SEED = 1100
# K = 15 / 16: a document that has taken 3 x 8 K records has more than 7 blocks on an interior level
# (ib_need + 8 K + 1 <= ib(K) asks for <= 7 at every K) and would leave for the class above -- at K = 16
# the LDS engine.  These two replay the K = 5 log, 40 of its records per launch, the rest non-ops.
B_REAL = {15: 40, 16: 40}
# K = 2 ... 4 (one apply at 32 records per launch): records per document after which some document has
# sat in each of the 128 / 192 / 256 bands at a launch's start and none has left the 320 class
SMALL_OPS = {('shrink', 8): 384, ('shrink', 48): 160, ('annotate', 16): 224, ('annotate', 48): 160,
             ('churn', 32): 160, ('churn', 48): 160}
B_STEPS = ('small',) + tuple(range(5, 17))


def n_clients(workload, form):
    return C64_CLIENTS if form == 'c64' else WORKLOADS[workload]['n_clients']


def step_launch(step):
    return 32 if step == 'small' else launch_size(step)


@functools.lru_cache(maxsize=None)
def workload(name, clients, step):
    """(batch, oracle, shapes): the log of one apply of part B ('small' or K = 5 ... 16), the oracle after
    it (events recorded) and the documents' doc_shape at the start of every launch"""
    oracle = _oracle()
    cfg = dict(WORKLOADS[name], n_clients=clients)
    n = step_launch(step)
    if step == 'small':
        batch = oracle.generate(N_DOCS, seed=SEED, ops_per_doc=SMALL_OPS[name, clients], **cfg)
    else:
        real = B_REAL.get(step, n)
        batch = oracle.generate(N_DOCS, seed=SEED + (5 if step in B_REAL else step), ops_per_doc=3 * real, **cfg)
        if real < n:
            batch = pad_launches(batch, real, n)
    o = oracle.Oracle(N_DOCS).record_events()
    shapes = []
    for part in batch.split_ops(n):
        shapes.append([doc_shape(o, d) for d in range(N_DOCS)])
        o.apply(part, threads=4)
    for d in range(N_DOCS):
        assert o.error(d) == (0, 0), (name, clients, step, d, o.error(d))
    return batch, o, shapes


def churn_arena(clients, step):
    """(text capacity, most inserted) of the churn documents: the smallest multiple of 1 KiB above twice
    the bytes the largest document inserts.  What is linked was inserted, so the arena half holds twice
    the linked text at every record (what a compaction plus a zamboni append's copy can need): "no
    arena error" is the only right outcome."""
    batch, _, _ = workload('churn', clients, step)
    most = max(inserted_bytes(batch, d) for d in range(N_DOCS))
    return (2 * most // 1024 + 1) * 1024, most


# ---- tight arenas in every class: text that turns over ---------------------------------------------
TURN_ARENA = 2048


@functools.lru_cache(maxsize=None)
def turnover(K, shift=0):
    """(batch, oracle, most linked text): 8 documents of 3 x launch_size(K) records, in cycles of three:
    a client inserts 120 ... 250 characters at the front, another removes all but the first two, a
    non-op message moves the msn past the removal (zamboni unlinks the tombstone and appends the
    two-character rests to one another).  Some 185 characters are written per cycle and at most a few
    hundred stay linked, so a 2 KiB arena half compacts every ten cycles or so."""
    from fluidframework_amd.oplog import build_batch
    n = launch_size(K)
    docs = []
    for d in range(N_DOCS):
        recs, seq = [], 0
        for j in range(n):  # 3 n records
            ln = 120 + (37 * j + 11 * d) % 131
            text = ''.join(chr(97 + (q * (3 + d) + j) % 26) for q in range(ln))
            for client, typ, p1, p2, tx in ((1 + (j + d) % 3, INSERT, 0, 0, text), (4 + j % 2, REMOVE, 2, ln, None),
                                            (1 + (j + d) % 3, NOOP, 0, 0, None)):
                seq += 1
                recs.append((seq, seq - 1, seq - 1, client + shift, typ, p1, p2, tx, None, 0))
        docs.append(recs)
    batch = build_batch(docs)
    oracle = _oracle()
    o, most = oracle.Oracle(N_DOCS), 0
    for part in batch.split_ops(1):
        o.apply(part, threads=4)
        most = max([most] + [linked_text(o, d) for d in range(N_DOCS)])
    ref = oracle.Oracle(N_DOCS).record_events().apply(batch, threads=4)
    for d in range(N_DOCS):
        assert ref.error(d) == (0, 0), (K, d, ref.error(d))
    return batch, ref, most


# ---- C. the error fixtures -------------------------------------------------------------------------
HALT_FIXTURES = ('errors', 'empty_inserts')


@functools.lru_cache(maxsize=None)
def halts(fixture, K):
    """(padded batch, oracle on it, the fixture's expectations)"""
    from conftest import load_golden
    batch, exp = load_golden(fixture)
    padded = pad_tail(batch, launch_size(K))
    o = _oracle().Oracle(padded.n_docs).record_events().apply(padded)
    return padded, o, exp
