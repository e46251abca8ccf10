// Host driver for tests/test_cpu_cluster_deal.py: compiles csrc/cluster_deal.hpp -- the very text tsp_cluster_run's pair table is
// built with -- and prints the table for every case on standard input.
//   case   = n ng C by_cost has_order scale, then ng * 4 box doubles, ng * 64 slot ints, 2n coordinate doubles, n order ints
//            (when has_order); doubles as C99 hex floats
//   answer = one line: ntests, then the C * ntests entries of the table
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "cluster_deal.hpp"

static double next_double() {
    double v;
    if (scanf("%lf", &v) != 1) { fprintf(stderr, "cluster_deal_check: input ends inside a case\n"); exit(2); }
    return v;
}

static int next_int() {
    int v;
    if (scanf("%d", &v) != 1) { fprintf(stderr, "cluster_deal_check: input ends inside a case\n"); exit(2); }
    return v;
}

int main() {
    int n;
    while (scanf("%d", &n) == 1) {
        const int ng = next_int(), C = next_int(), by_cost = next_int(), has_order = next_int();
        const double scale = next_double();
        if (n < 1 || ng < 1 || ng > 32768 || C < 1) { fprintf(stderr, "cluster_deal_check: bad case header\n"); return 2; }
        std::vector<double> gbox((size_t)ng * 4), xy((size_t)n * 2);
        std::vector<int> sperm((size_t)ng * 64), order;
        for (double &v : gbox) v = next_double();
        for (int &v : sperm) v = next_int();
        for (double &v : xy) v = next_double();
        if (has_order) { order.resize((size_t)n); for (int &v : order) v = next_int(); }
        std::vector<int> tab;
        const long long ntests = tsp::cluster_deal(gbox.data(), sperm.data(), xy.data(), has_order ? order.data() : nullptr, n, ng, C,
                                                   by_cost != 0, scale, tab);
        if ((long long)tab.size() != ntests * C) { fprintf(stderr, "cluster_deal_check: table of %zu entries\n", tab.size()); return 3; }
        printf("%lld", ntests);
        for (int v : tab) printf(" %d", v);
        printf("\n");
    }
    return 0;
}
