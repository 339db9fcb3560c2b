// mt_scratch.h -- the host-to-device round trip of a query entry, in three pieces:
//   mt_layout   the byte offsets of the parts of one scratch block (plain host C++, no HIP)
//   mt_scratch  the block on the device: one hipMalloc, freed with the object
//   mt_chain    the copies, launches and the synchronisation on one stream; after the first failure
//               the later steps do nothing
// A wrapper reads: argument check, layout, chain, return.  Nothing is pooled or cached: every call
// allocates its scratch and frees it.
//
// With MT_SCRATCH_LAYOUT_ONLY defined only the first piece (and the host helpers next to it) is
// declared, and no HIP header is needed (tests/test_scratch_layout_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Parts of one block, each starting on a 16-byte boundary (a 12-byte record in front of a 16-byte
// one leaves the second aligned whatever the count).  add<T>(count) returns the part's byte offset;
// a part of no elements takes no room.  A byte size or a total past SIZE_MAX marks the layout bad.
struct mt_layout {
    size_t total = 0;
    bool bad = false;
    template <class T>
    size_t add(size_t count) {
        const size_t off = total;
        const size_t bytes = (count * sizeof(T) + 15) & ~size_t(15);
        if (count > (SIZE_MAX - 15) / sizeof(T) || bytes > SIZE_MAX - total) bad = true;
        else total += bytes;
        return off;
    }
};

// Rows from counts: row_ptr[0 .. n] = the prefix sums of count(0 .. n - 1), *total their sum.  A sum
// that reaches 2^32 is refused (false): *total is left alone and the rows are not to be used.
template <class Count>
bool mt_rows_from_counts(uint32_t n, Count count, uint32_t* row_ptr, uint64_t* total) {
    uint64_t sum = 0;
    row_ptr[0] = 0;
    for (uint32_t i = 0; i < n; i++) {
        sum += count(i);
        if (sum >= (1ull << 32)) return false;
        row_ptr[i + 1] = (uint32_t)sum;
    }
    *total = sum;
    return true;
}

// every document named by a batch of queries exists: records with a `doc` field, or plain ids
template <class T>
bool mt_docs_below(const T* q, uint32_t n, uint32_t n_docs) {
    for (uint32_t i = 0; i < n; i++)
        if (q[i].doc >= n_docs) return false;
    return true;
}
inline bool mt_docs_below(const uint32_t* docs, uint32_t n, uint32_t n_docs) {
    for (uint32_t i = 0; i < n; i++)
        if (docs[i] >= n_docs) return false;
    return true;
}

// The batch of mt_refs_insert_local (include/mtgpu.h): every document known and the documents strictly
// ascending (one insert per document), every record a local INSERT (seq -1, type 0) whose payload
// lies inside payload_bytes.  true: rows[0 .. n_docs] is the batch's row pointer -- record i is row i,
// its document's only one.  false: refused, rows is not to be used.
template <class At, class Op>
bool mt_ref_insert_rows(const At* at, const Op* ops, uint32_t n, uint32_t n_docs, uint64_t payload_bytes, uint32_t* rows) {
    for (uint32_t i = 0; i < n; i++) {
        if (at[i].doc >= n_docs || (i && at[i].doc <= at[i - 1].doc)) return false;
        if (ops[i].seq != -1 || ops[i].type != 0) return false;
        if ((uint64_t)ops[i].payload_off + ops[i].payload_len > payload_bytes) return false;
    }
    uint32_t i = 0;
    rows[0] = 0;
    for (uint32_t d = 0; d < n_docs; d++) {
        if (i < n && at[i].doc == d) i++;
        rows[d + 1] = i;
    }
    return true;
}

#ifndef MT_SCRATCH_LAYOUT_ONLY
#include <hip/hip_runtime.h>

#include <tuple>
#include <utility>

#include "../../include/mtgpu.h"

// The block of a layout on the current device.  carve<T...>(counts...) lays out one part per type,
// allocates the block (once per object) and returns the parts' pointers:
//     auto [dq, dr] = s.carve<mt_tile_query, mt_tile_result>(n, n);
// A bad layout or a failed allocation: status() is MT_ERR_NOMEM and the pointers are not to be used
// (a chain started from status() never does).
class __attribute__((visibility("hidden"))) mt_scratch {
public:
    mt_scratch() = default;
    ~mt_scratch() {
        if (p_) (void)hipFree(p_);
    }
    mt_scratch(const mt_scratch&) = delete;
    mt_scratch& operator=(const mt_scratch&) = delete;
    template <class... T>
    std::tuple<T*...> carve(decltype(sizeof(T))... counts) {
        mt_layout l;
        const size_t off[] = {l.add<T>(counts)...};
        if (l.bad || hipMalloc(&p_, l.total ? l.total : 1) != hipSuccess) p_ = nullptr;
        size_t i = 0;
        return std::tuple<T*...>{at<T>(off[i++])...};
    }
    mt_status status() const { return p_ ? MT_OK : MT_ERR_NOMEM; }
    template <class T>
    T* at(size_t off) const {
        return reinterpret_cast<T*>(static_cast<uint8_t*>(p_) + off);
    }

private:
    void* p_ = nullptr;
};

// Steps on one stream behind a sticky status.  launch(f, args...) calls a function that returns
// hipError_t (a launcher of mt_launch.h, a HIP call), call(f, args...) one that returns mt_status (a
// *_device entry): the function is not called once a step has failed.  A HIP failure is MT_ERR_HIP,
// a call's failure keeps its own code.  Copies of no bytes are skipped.
class __attribute__((visibility("hidden"))) mt_chain {
public:
    explicit mt_chain(hipStream_t stream, mt_status start = MT_OK) : stream_(stream), st_(start) {}
    mt_chain& h2d(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyHostToDevice); }
    mt_chain& d2h(void* dst, const void* src, size_t bytes) { return copy(dst, src, bytes, hipMemcpyDeviceToHost); }
    template <class F, class... A>
    mt_chain& launch(F f, A&&... a) {
        if (st_ == MT_OK && f(std::forward<A>(a)...) != hipSuccess) st_ = MT_ERR_HIP;
        return *this;
    }
    template <class F, class... A>
    mt_chain& call(F f, A&&... a) {
        if (st_ == MT_OK) st_ = f(std::forward<A>(a)...);
        return *this;
    }
    mt_chain& sync() { return launch(hipStreamSynchronize, stream_); }
    mt_status status() const { return st_; }

private:
    mt_chain& copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        return bytes ? launch(hipMemcpyAsync, dst, src, bytes, kind, stream_) : *this;
    }
    hipStream_t stream_;
    mt_status st_;
};
#endif  // MT_SCRATCH_LAYOUT_ONLY
