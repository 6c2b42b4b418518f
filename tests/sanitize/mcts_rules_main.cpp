// mcts_rules_main.cpp — the rules-MCTS opponent's header
// (muzero.jl_amd/csrc/mz_mcts_rules.h) as a stand-alone CPU program, built
// with -fsanitize=address,undefined by tests/test_mcts_rules_host.py.
//
// Input file, one position per line:  env player sims rollouts seed id rng_step planes
//   env 0 = TicTacToe, 1 = Connect4; planes = the [p1, p2, empty] bytes as a
//   string of '0' / '1' (27 or 126 of them).
// Output, one line per position: the A counts n, then the A sums w, separated
// by blanks, or "rejected" for what mz_mcts_eval refuses (a cell in no plane
// or in more than one, a player outside 1..2, sims outside 1..1024, rollouts
// outside 1..64, a malformed line).
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../muzero.jl_amd/csrc/mz_mcts_rules.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s positions.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string line;
    long n = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++n;
        std::istringstream ls(line);
        int env = -1, player = 0, sims = 0, rollouts = 0;
        unsigned long long seed = 0;
        unsigned long id = 0, rng_step = 0;
        std::string planes;
        ls >> env >> player >> sims >> rollouts >> seed >> id >> rng_step >> planes;
        bool ok = !ls.fail() && (env == MZX_TICTACTOE || env == MZX_CONNECT4) && sims >= 1 && sims <= MZM_MAX_SIMS &&
                  rollouts >= 1 && rollouts <= MZM_MAX_ROLLOUTS;
        std::vector<uint8_t> b;
        if (ok) {
            ok = planes.size() == (size_t)(3 * mzx_cells(env));
            for (char c : planes) {
                ok = ok && (c == '0' || c == '1');
                b.push_back(c == '1');
            }
        }
        ExpertPos pos;
        if (!ok || !mzx_pos_from_planes(env, b.data(), player, &pos)) {
            std::cout << "rejected\n";
            continue;
        }
        // every array has exactly the size the header documents: an access past it is the sanitizer's to find
        const int A = mzx_actions(env);
        std::vector<double> sqrt_tab(sims + 1);
        for (size_t k = 0; k < sqrt_tab.size(); ++k) sqrt_tab[k] = std::sqrt((double)k);
        std::vector<int32_t> nn(A), ww(A);
        mcts_root_stats(pos, sims, rollouts, (uint64_t)seed, (uint32_t)id, (uint32_t)rng_step, sqrt_tab.data(),
                        nn.data(), ww.data());
        for (int a = 0; a < A; ++a) std::cout << (a ? " " : "") << nn[a];
        for (int a = 0; a < A; ++a) std::cout << " " << ww[a];
        std::cout << "\n";
    }
    std::cerr << "mcts_rules_main: " << n << " positions\n";
    return 0;
}
