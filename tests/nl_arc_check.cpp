// nl_arc_check.cpp -- csrc/nl_arc.hpp as the kernels of the batched list descent include it, built with the host compiler and driven
// from standard input by tests/test_cpu_nl_batch.py.  One answer line per command line:
//   arc n key pos[0] .. pos[n-1]      -> "start len" of nl_arc_of_key
//   two n pi pj | three n pa pc | or n pf pa L   -> "start len" of the kind's own function
//   disj n s1 l1 s2 l2                -> 1 when the arcs are disjoint, else 0, from nl_arc_disjoint and, position by position, from
//                                        nl_arc_holds: "d h"
//   key n a b c type                  -> "k a b c type": k = nl3_key(a, b, c, type, n) and what nl3_unkey(k, n) gives back
#include "nl_arc.hpp"

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        int n = 0;
        in >> cmd >> n;
        if (cmd == "arc") {
            unsigned long long key = 0;
            in >> key;
            std::vector<int> pos((size_t)n);
            for (int &p : pos) in >> p;
            const tsp::NlArc a = tsp::nl_arc_of_key(pos.data(), n, key);
            std::cout << a.start << " " << a.len << "\n";
        } else if (cmd == "two" || cmd == "three") {
            int p = 0, q = 0;
            in >> p >> q;
            const tsp::NlArc a = cmd == "two" ? tsp::nl_arc_two(p, q, n) : tsp::nl_arc_three(p, q, n);
            std::cout << a.start << " " << a.len << "\n";
        } else if (cmd == "or") {
            int pf = 0, pa = 0, L = 0;
            in >> pf >> pa >> L;
            const tsp::NlArc a = tsp::nl_arc_or(pf, pa, L, n);
            std::cout << a.start << " " << a.len << "\n";
        } else if (cmd == "key") {
            int a = 0, b = 0, c = 0, type = 0;
            in >> a >> b >> c >> type;
            const unsigned long long k = tsp::nl3_key(a, b, c, type, n);
            const tsp::Nl3Move m = tsp::nl3_unkey(k, n);
            std::cout << k << " " << m.a() << " " << m.b() << " " << m.c() << " " << m.type() << "\n";
        } else if (cmd == "disj") {
            tsp::NlArc x{0, 0}, y{0, 0};
            in >> x.start >> x.len >> y.start >> y.len;
            bool shared = false;
            for (int p = 0; p < n; ++p) shared = shared || (tsp::nl_arc_holds(x, p, n) && tsp::nl_arc_holds(y, p, n));
            std::cout << (tsp::nl_arc_disjoint(x, y, n) ? 1 : 0) << " " << (shared ? 0 : 1) << "\n";
        } else {
            std::cout << "?\n";
        }
        if (!in) return 2;
    }
    return 0;
}
