// expert_rules_main.cpp — the expert opponent's rules header
// (muzero.jl_amd/csrc/mz_expert_rules.h) as a stand-alone CPU program, built
// with -fsanitize=address,undefined by tests/test_expert_rules_host.py.
//
// Input file, one position per line:  env player depth planes
//   env 0 = TicTacToe, 1 = Connect4; planes = the [p1, p2, empty] bytes as a
//   string of '0' / '1' (27 or 126 of them).
// Output, one line per position: the A scores separated by blanks, or
// "rejected" for what mz_expert_eval refuses (a cell in no plane or in more
// than one, a player outside 1..2, a depth outside 1..9, a malformed line).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../muzero.jl_amd/csrc/mz_expert_rules.h"

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
        int env = -1, player = 0, depth = 0;
        std::string planes;
        ls >> env >> player >> depth >> planes;
        bool ok = !ls.fail() && (env == MZX_TICTACTOE || env == MZX_CONNECT4) && depth >= 1 && depth <= MZX_MAX_DEPTH;
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
        int32_t sc[9];
        expert_scores(pos, depth, sc);
        for (int a = 0; a < mzx_actions(env); ++a) std::cout << (a ? " " : "") << sc[a];
        std::cout << "\n";
    }
    std::cerr << "expert_rules_main: " << n << " positions\n";
    return 0;
}
