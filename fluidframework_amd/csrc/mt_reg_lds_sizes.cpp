// mt_reg_lds_sizes.cpp -- stand-alone host program: "K sizeof(RLds<K>)" for K = 2 .. 16, one per line
// (tools/resource_usage.py writes them into profiles/rNN_resource_usage_reg.txt;
// tests/test_reg_lds_layout.py pins them).  Not part of libmtgpu.so.
#include <cstdio>

#include "mt_reg_lds.h"

template <int K>
static void row() {
    std::printf("%d %zu\n", K, sizeof(mtr::RLds<K>));
    if constexpr (K < 16) row<K + 1>();
}

int main() { row<2>(); }
