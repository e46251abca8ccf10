// Host driver for tests/test_cpu_exh_deal.py: compiles csrc/exh_arith.hpp -- the very text tsp_dev_tours_create fills k_exh's
// table of descriptors with, and whose exh_strip k_exh walks the strips with -- and prints the descriptors of every wave for every
// case on standard input.
//   case   = n weff waves_total share0 share1 share2 share3 gens
//   answer = one line: strips, total, then strips x (q0 rows), then waves_total x (strip row count)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "exh_arith.hpp"

int main() {
    int n, weff, waves_total, share[4], gens;
    while (scanf("%d %d %d %d %d %d %d %d", &n, &weff, &waves_total, &share[0], &share[1], &share[2], &share[3], &gens) == 8) {
        if (n < 5 || weff < 1 || waves_total < 1 || gens < 0 || gens > 4 || (share[0] > 0 && gens > waves_total)) {
            fprintf(stderr, "exh_deal_check: bad case\n");
            return 2;
        }
        const int strips = tsp::exh_strips(n, weff);
        printf("%d %lld", strips, tsp::exh_total_rows(n, weff));
        for (int s = 0; s < strips; ++s) {
            const tsp::ExhStrip st = tsp::exh_strip(n, weff, s);
            printf(" %d %d", st.q0, st.rows);
        }
        std::vector<tsp::ExhDeal> tab((size_t)waves_total);   // as the host fills it
        for (int gw = 0; gw < waves_total; ++gw) tab[(size_t)gw] = tsp::exh_deal(n, weff, waves_total, share, gens, gw);
        for (const tsp::ExhDeal &d : tab) printf(" %d %d %lld", d.strip, d.row, d.count);
        printf("\n");
    }
    return 0;
}
