// Host check of sgp_out_message's scratch layout (layout_out_message, gaussianprocessnode_amd/csrc/point_scratch.h), in the style of
// tools/point_scratch_check.cpp: over a grid of shapes the pieces are pairwise disjoint at the sizes their consumers need (stated
// here independently of the layout function), every piece starts a multiple of Carver::ALIGN doubles from the base, pass 2 hands
// out the total pass 1 summed, and every piece can be written end to end inside the allocation.  No GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -o tools/out_message_scratch_check tools/out_message_scratch_check.cpp
//   && tools/out_message_scratch_check
#include "../gaussianprocessnode_amd/csrc/point_scratch.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {
struct Piece { const char* name; void* p; size_t bytes; };
long failures = 0;
void fail(const PointShape& s, size_t mu, const char* what, const char* name) {
    if (++failures <= 20)
        std::fprintf(stderr, "D %d d_out %d chunk %lld n %lld nodes %lld mu %zu: %s %s\n", s.D, s.dout, (long long)s.chunk,
                     (long long)s.n, (long long)s.n_nodes, mu, what, name);
}
}  // namespace

int main() {
    long shapes = 0;
    for (int D : {1, 2, 5, 32})
        for (int dout = 1; dout <= 4; ++dout)
            for (long long n : {1LL, 5LL, 63LL, 64LL, 65LL, 158LL, 1500LL})
                for (long long nodes : {1LL, 3LL, n})
                    for (long long chunk : {64LL, 128LL, (n + 63) / 64 * 64})
                        for (size_t mu : {(size_t)0, (size_t)dout * 48, (size_t)dout * 130}) {
                            if (nodes > n) continue;
                            const PointShape s{0, 0, 0, D, dout, 0, chunk, n, nodes};
                            Carver c;
                            OutMessageScratch b;
                            layout_out_message(c, s, mu, &b);
                            const size_t total = c.used;
                            std::vector<double> mem(total + 1);
                            c = Carver{mem.data()};
                            layout_out_message(c, s, mu, &b);
                            if (c.used != total) fail(s, mu, "pass 2 handed out another total than pass 1 summed", "");
                            const size_t d = sizeof(double);
                            std::vector<Piece> pieces = {
                                {"Xall", b.Xall, (size_t)n * D * d}, {"PointMean", b.PointMean, (size_t)n * dout * d},
                                {"Wt", b.Wt, (size_t)n * d}, {"MeanC", b.MeanC, (size_t)chunk * dout * d},
                                {"Start", b.Start, (size_t)(nodes + 1) * sizeof(int64_t)}, {"MeanN", b.MeanN, (size_t)nodes * dout * d},
                                {"Mu", b.Mu, mu * d}};
                            const char* lo = reinterpret_cast<const char*>(mem.data());
                            for (const Piece& p : pieces) std::memset(p.p, 0x5a, p.bytes);      // (the sanitizer sees a write past the end)
                            std::sort(pieces.begin(), pieces.end(), [](const Piece& x, const Piece& y) { return x.p < y.p; });
                            for (size_t i = 0; i < pieces.size(); ++i) {
                                const char* p = static_cast<const char*>(pieces[i].p);
                                if (p < lo || (size_t)(p - lo) % (Carver::ALIGN * d) != 0) fail(s, mu, "misaligned:", pieces[i].name);
                                const char* next = i + 1 < pieces.size() ? static_cast<const char*>(pieces[i + 1].p) : lo + total * d;
                                if (p + pieces[i].bytes > next) fail(s, mu, "overlap or past the total:", pieces[i].name);
                            }
                            ++shapes;
                        }
    std::printf("%ld shapes, %ld failures\n", shapes, failures);
    return failures ? 1 : 0;
}
