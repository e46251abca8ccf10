// Host driver for tests/test_cpu_row_scan.py: compiles the HIP-free part of csrc/row_scan.hpp -- the very text the row-scan
// kernels and their host code compile -- and answers the commands on standard input, one line of output each:
//   chunks n waves max min        -> CH Cc                                   (scan_chunks)
//   fewrows n max min             -> CH Cc                                   (scan_chunks_few_rows)
//   edges count want  (lo hi) x count
//                                 -> returned number, then the 2 * want values of edges[] (preset to -7)
//   carve k  (size count) x k     -> total, then the k offsets from the base    (size in {1, 4, 8, 16, 32})
//   finite m  values              -> 0 / 1                                   (pi_finite; m = 0: NULL)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "row_scan.hpp"

using namespace tsp;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "chunks") {
            int n, w, mx, mn;
            std::cin >> n >> w >> mx >> mn;
            const ScanChunks g = scan_chunks(n, w, mx, mn);
            std::printf("%d %d\n", g.CH, g.Cc);
        } else if (cmd == "fewrows") {
            int n, mx, mn;
            std::cin >> n >> mx >> mn;
            const ScanChunks g = scan_chunks_few_rows(n, mx, mn);
            std::printf("%d %d\n", g.CH, g.Cc);
        } else if (cmd == "edges") {
            int count, want;
            std::cin >> count >> want;
            std::vector<int> lo((size_t)count), hi((size_t)count), edges(2 * (size_t)want, -7);
            for (int k = 0; k < count; ++k) std::cin >> lo[(size_t)k] >> hi[(size_t)k];
            std::printf("%d", write_sorted_edges(lo.data(), hi.data(), count, edges.data(), want));
            for (int v : edges) std::printf(" %d", v);
            std::printf("\n");
        } else if (cmd == "carve") {
            int k;
            std::cin >> k;
            std::vector<int> size((size_t)k);
            std::vector<size_t> count((size_t)k);
            for (int i = 0; i < k; ++i) std::cin >> size[(size_t)i] >> count[(size_t)i];
            struct alignas(32) B32 { char b[32]; };
            struct alignas(16) B16 { char b[16]; };
            std::vector<char *> at((size_t)k, nullptr);
            auto lay = [&](Carver &c) {
                for (int i = 0; i < k; ++i) {
                    char *&p = at[(size_t)i];
                    switch (size[(size_t)i]) {
                    case 1: c(p, count[(size_t)i]); break;
                    case 4: { int *q = nullptr; c(q, count[(size_t)i]); p = reinterpret_cast<char *>(q); } break;
                    case 8: { double *q = nullptr; c(q, count[(size_t)i]); p = reinterpret_cast<char *>(q); } break;
                    case 16: { B16 *q = nullptr; c(q, count[(size_t)i]); p = reinterpret_cast<char *>(q); } break;
                    default: { B32 *q = nullptr; c(q, count[(size_t)i]); p = reinterpret_cast<char *>(q); } break;
                    }
                }
            };
            const size_t total = carve_bytes(lay);
            char *base = static_cast<char *>(std::aligned_alloc(256, total ? total : 256));
            carve(base, lay);
            std::printf("%zu", total);
            for (int i = 0; i < k; ++i) {
                if (count[(size_t)i]) std::memset(at[(size_t)i], i, (size_t)size[(size_t)i] * count[(size_t)i]);   // inside the block
                std::printf(" %td", at[(size_t)i] - base);
            }
            std::printf(" %d\n", (int)(reinterpret_cast<uintptr_t>(at.empty() ? base : at[0]) % 256));
            std::free(base);
        } else if (cmd == "finite") {
            int m;
            std::cin >> m;
            std::vector<double> v((size_t)m);
            for (auto &x : v) { std::string t; std::cin >> t; x = std::strtod(t.c_str(), nullptr); }
            std::printf("%d\n", pi_finite(m ? v.data() : nullptr, m) ? 1 : 0);
        } else {
            std::fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
