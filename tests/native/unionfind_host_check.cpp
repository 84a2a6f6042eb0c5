// Host check of csrc/unionfind.h (the merge structure of revo_gallery_clusters): 8 threads apply shuffled shares of edge
// lists -- chains, stars, a dense clique, duplicate edges, self-pairs, random edges -- through uf_unite at once; afterwards
// uf_find of every vertex must equal a sequential union-find's minimum-of-component, parent[x] <= x must hold, every root
// must be the minimum of its component, and the error word must be 0.  Built with -fsanitize=address,undefined (Makefile
// target unionfind_check); prints ALL OK.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "../../revers-o_amd/csrc/unionfind.h"

namespace {
using Edge = std::pair<uint32_t, uint32_t>;

struct SeqUf {
    std::vector<uint32_t> p;
    explicit SeqUf(uint32_t n) : p(n) { for (uint32_t i = 0; i < n; ++i) p[i] = i; }
    uint32_t find(uint32_t x) { while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; } return x; }
    void unite(uint32_t a, uint32_t b) {
        a = find(a); b = find(b);
        if (a != b) p[std::max(a, b)] = std::min(a, b);
    }
};

int run_case(const char* name, uint32_t n, std::vector<Edge> edges, unsigned seed) {
    const int T = 8;
    std::mt19937 rng(seed);
    std::shuffle(edges.begin(), edges.end(), rng);
    std::vector<uint32_t> parent(n);
    for (uint32_t i = 0; i < n; ++i) parent[i] = i;
    uint32_t err = 0;
    const revo::UfLimits lim = revo::uf_limits((long)n);
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t)
        th.emplace_back([&, t]() {
            // thread t: every T-th edge, and (half of the threads) the whole list once more backwards -- repeated unions
            for (size_t e = (size_t)t; e < edges.size(); e += T) revo::uf_unite(parent.data(), edges[e].first, edges[e].second, lim, &err);
            if (t & 1)
                for (size_t e = edges.size(); e-- > 0;) revo::uf_unite(parent.data(), edges[e].second, edges[e].first, lim, &err);
        });
    for (auto& t : th) t.join();
    SeqUf ref(n);
    for (const Edge& e : edges) ref.unite(e.first, e.second);
    int bad = 0;
    if (err != 0) { std::printf("%s: error word set\n", name); ++bad; }
    for (uint32_t x = 0; x < n && bad < 10; ++x) {
        if (parent[x] > x) { std::printf("%s: parent[%u] = %u > %u\n", name, x, parent[x], x); ++bad; }
        const uint32_t want = ref.find(x);                  // the sequential root is the component's minimum as well
        if (parent[x] == x && want != x) { std::printf("%s: root %u is not the minimum %u of its component\n", name, x, want); ++bad; }
    }
    for (uint32_t x = 0; x < n && bad < 10; ++x) {
        const uint32_t got = revo::uf_find(parent.data(), x, lim.walk, &err), want = ref.find(x);
        if (got != want) { std::printf("%s: find(%u) = %u, expected %u\n", name, x, got, want); ++bad; }
    }
    if (err != 0 && bad == 0) { std::printf("%s: error word set by find\n", name); ++bad; }
    std::printf("%-28s n = %7u  edges = %8zu  %s\n", name, n, edges.size(), bad ? "FAILED" : "ok");
    return bad;
}
}  // namespace

int main() {
    int bad = 0;
    std::mt19937 rng(12345);
    {   // one chain over every vertex, ascending, and one descending through a permutation
        const uint32_t n = 200000;
        std::vector<Edge> e;
        for (uint32_t i = 0; i + 1 < n; ++i) e.emplace_back(i, i + 1);
        bad += run_case("chain ascending", n, e, 1);
        std::vector<uint32_t> perm(n);
        for (uint32_t i = 0; i < n; ++i) perm[i] = i;
        std::shuffle(perm.begin(), perm.end(), rng);
        e.clear();
        for (uint32_t i = 0; i + 1 < n; ++i) e.emplace_back(perm[i + 1], perm[i]);
        bad += run_case("chain permuted", n, e, 2);
    }
    {   // stars: centre at the highest, the lowest and a middle index of each block of 1000
        const uint32_t n = 100000;
        std::vector<Edge> e;
        for (uint32_t b = 0; b + 1000 <= n; b += 1000) {
            const uint32_t c = b + ((b / 1000) % 3 == 0 ? 999 : ((b / 1000) % 3 == 1 ? 0 : 500));
            for (uint32_t i = b; i < b + 1000; ++i) if (i != c) e.emplace_back(c, i);
        }
        bad += run_case("stars", n, e, 3);
    }
    {   // a dense clique (every pair), twice over, with self-pairs, inside a larger vertex set
        const uint32_t n = 5000, m = 1200, off = 777;
        std::vector<Edge> e;
        for (uint32_t i = 0; i < m; ++i)
            for (uint32_t j = i + 1; j < m; ++j) { e.emplace_back(off + i, off + j); e.emplace_back(off + j, off + i); }
        for (uint32_t i = 0; i < n; ++i) e.emplace_back(i, i);
        bad += run_case("clique + duplicates + self", n, e, 4);
    }
    {   // random sparse graphs around the connectivity threshold: many components of every size
        for (int rep = 0; rep < 3; ++rep) {
            const uint32_t n = 300000;
            std::uniform_int_distribution<uint32_t> d(0, n - 1);
            std::vector<Edge> e;
            const size_t m = (size_t)n * (rep + 1) / 3;
            for (size_t i = 0; i < m; ++i) e.emplace_back(d(rng), d(rng));
            bad += run_case("random sparse", n, e, 10 + rep);
        }
    }
    {   // the smallest sets
        bad += run_case("one vertex", 1, {Edge(0, 0)}, 20);
        bad += run_case("two vertices", 2, {Edge(1, 0), Edge(0, 1), Edge(1, 1)}, 21);
    }
    if (bad) { std::printf("FAILED\n"); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
