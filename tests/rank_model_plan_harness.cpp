// rank_model_plan_harness.cpp — drives spaghettisearch_amd/csrc/rank_model_plan.hpp on the host (tests/test_rank_model_cpu.py compiles
// it with ASan + UBSan).  One command per input line, one answer line each, "ok <lines> lines" at the end.  Arrays are allocated at
// their exact sizes so that a read past an end is a sanitizer report.
//   m <n_features> <base> <L> <linear x L> <n_trees> <tree_ptr x (n_trees + 1)> <N> <feature left right nan_left value> x N
//        -> <code> <n_nodes> <max_tree_nodes> <max_depth>          (check_model; L = 0: linear NULL)
//   c <cap> <n_trees> <tree_ptr x (n_trees + 1)>
//        -> the chunks, each first_tree:n_trees:first_node:n_nodes:global
//   p <feature> <left> <right> <nan_left>
//        -> <is_leaf> <feature> <left> <right> <nan_left>           (pack_link and the accessors)
//   k <value>  -> clamp_cap(value)
#include "rank_model_plan.hpp"

#include <cstdlib>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

namespace rp = ss::rankp;

static double num(std::istringstream& in) {
    std::string w;
    in >> w;
    return std::strtod(w.c_str(), nullptr);             // "nan", "inf", "-inf" included
}

int main() {
    std::string line;
    size_t lines = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        char cmd = 0;
        in >> cmd;
        if (cmd == 'm') {
            int32_t nf = 0, n_trees = 0;
            size_t L = 0, N = 0;
            in >> nf;
            const double base = num(in);
            in >> L;
            std::unique_ptr<double[]> linear(L ? new double[L] : nullptr);
            for (size_t i = 0; i < L; i++) linear[i] = num(in);
            in >> n_trees;
            const size_t np = n_trees >= 0 ? (size_t)n_trees + 1 : 0;
            std::unique_ptr<uint32_t[]> ptr(new uint32_t[np ? np : 1]);
            for (size_t i = 0; i < np; i++) in >> ptr[i];
            in >> N;
            std::unique_ptr<rp::Node[]> nodes(N ? new rp::Node[N] : nullptr);
            for (size_t i = 0; i < N; i++) {
                in >> nodes[i].feature >> nodes[i].left >> nodes[i].right >> nodes[i].nan_left;
                nodes[i].value = num(in);
            }
            char msg[256] = "";
            rp::Info info{};
            const int rc = rp::check_model(msg, sizeof(msg), "harness", nf, linear.get(), base, n_trees, ptr.get(), nodes.get(), &info);
            if (rc == rp::OK && N) {                    // a model that passes is packed, as create does
                std::unique_ptr<rp::PNode[]> packed(new rp::PNode[N]);
                rp::pack_nodes(nodes.get(), N, packed.get());
                for (size_t i = 0; i < N; i++)
                    if (rp::link_is_leaf(packed[i].link) != (nodes[i].feature < 0)) return 3;
            }
            std::cout << rc << " " << info.n_nodes << " " << info.max_tree_nodes << " " << info.max_depth << "\n";
        } else if (cmd == 'c') {
            uint32_t cap = 0, n_trees = 0;
            in >> cap >> n_trees;
            std::unique_ptr<uint32_t[]> ptr(new uint32_t[n_trees + 1]);
            for (uint32_t i = 0; i <= n_trees; i++) in >> ptr[i];
            const std::vector<rp::Chunk> cs = rp::chunks(ptr.get(), n_trees, cap);
            for (size_t i = 0; i < cs.size(); i++)
                std::cout << (i ? " " : "") << cs[i].first_tree << ":" << cs[i].n_trees << ":" << cs[i].first_node << ":" << cs[i].n_nodes << ":" << (cs[i].global ? 1 : 0);
            std::cout << "\n";
        } else if (cmd == 'p') {
            int32_t f = 0;
            uint32_t l = 0, r = 0, nl = 0;
            in >> f >> l >> r >> nl;
            const uint64_t link = rp::pack_link(f, l, r, nl);
            if (rp::link_is_leaf(link)) std::cout << "1 -1 0 0 0\n";
            else std::cout << "0 " << rp::link_feature(link) << " " << rp::link_left(link) << " " << rp::link_right(link) << " " << (rp::link_nan_left(link) ? 1 : 0) << "\n";
        } else if (cmd == 'k') {
            long long v = 0;
            in >> v;
            std::cout << rp::clamp_cap(v) << "\n";
        } else {
            return 2;
        }
        lines++;
    }
    std::cout << "ok " << lines << " lines\n";
    return 0;
}
