// expert_table_main.cpp — the solved TicTacToe table's host side
// as a stand-alone CPU program, built with -fsanitize=address,undefined by
// tests/test_expert_table.py: mzx_ttt_code and its inverse from
// muzero.jl_amd/csrc/mz_expert_rules.h over all 19683 codes, and a table
// filled by the header's expert_scores in the device's 16-byte entry layout.
//
// Input file: one table code per line.
// Output: "roundtrip ok" (or the first code that fails), then one line per
// input code: the code and its nine depth-9 scores, or "rejected" for a code
// outside the table or a malformed line.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../muzero.jl_amd/csrc/mz_expert_rules.h"

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s codes.txt\n", argv[0]);
        return 2;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    // code -> position -> code, and through the byte planes as either player
    int bad = -1;
    for (int code = 0; code < MZX_TTT_CODES && bad < 0; ++code) {
        const ExpertPos pos = mzx_ttt_decode(code);
        if ((pos.me & pos.opp) || ((pos.me | pos.opp) >> 9) || pos.env != MZX_TICTACTOE || mzx_ttt_code(pos) != code)
            bad = code;
        for (int player = 1; player <= 2 && bad < 0; ++player) {
            uint8_t planes[27];
            for (int c = 0; c < 9; ++c) {
                const int me = (int)((pos.me >> c) & 1), opp = (int)((pos.opp >> c) & 1);
                planes[c] = (uint8_t)(player == 1 ? me : opp);
                planes[9 + c] = (uint8_t)(player == 1 ? opp : me);
                planes[18 + c] = (uint8_t)(1 - me - opp);
            }
            ExpertPos back;
            if (!mzx_pos_from_planes(MZX_TICTACTOE, planes, player, &back) || back.me != pos.me ||
                back.opp != pos.opp || mzx_ttt_code(back) != code)
                bad = code;
        }
    }
    if (bad < 0) std::cout << "roundtrip ok\n";
    else std::cout << "roundtrip fails at " << bad << "\n";
    // the table, as the device holds it
    std::vector<int8_t> table((size_t)MZX_TTT_CODES * MZX_TTT_ENTRY, (int8_t)MZX_ILLEGAL);
    for (int code = 0; code < MZX_TTT_CODES; ++code) {
        int32_t sc[9];
        expert_scores(mzx_ttt_decode(code), MZX_MAX_DEPTH, sc);
        for (int a = 0; a < 9; ++a) table[(size_t)code * MZX_TTT_ENTRY + a] = (int8_t)sc[a];
    }
    std::string line;
    long n = 0;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        ++n;
        std::istringstream ls(line);
        long code = -1;
        ls >> code;
        if (ls.fail() || code < 0 || code >= MZX_TTT_CODES) {
            std::cout << "rejected\n";
            continue;
        }
        std::cout << code;
        for (int a = 0; a < 9; ++a) std::cout << " " << (int)table[(size_t)code * MZX_TTT_ENTRY + a];
        std::cout << "\n";
    }
    std::cerr << "expert_table_main: " << n << " codes\n";
    return 0;
}
