// prior_rules_main.cpp — the network-only player's header
// (muzero.jl_amd/csrc/mz_prior_rules.h) as a stand-alone CPU program, built
// with -fsanitize=address,undefined by tests/test_prior_rules_host.py.
//
// Input file, one row per line:  A T r mask p[0] .. p[A-1]
//   T and every p[a] = the float's bits in hex; r = the ACTION draw (decimal);
//   mask = the legal bytes as a string of '0' / '1' (A of them).
// Output, one line per row: the 0-based action, then π's bits in hex,
// separated by blanks, or "rejected" for what mzp_row refuses (an empty legal
// set, A outside 1..32, a negative or NaN temperature) and for a malformed line.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../muzero.jl_amd/csrc/mz_prior_rules.h"

static bool hex_float(const std::string& s, float* out) {
    if (s.size() != 8) return false;
    char* end = nullptr;
    const unsigned long u = std::strtoul(s.c_str(), &end, 16);
    if (*end) return false;
    const uint32_t b = (uint32_t)u;
    std::memcpy(out, &b, 4);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        std::fprintf(stderr, "usage: %s rows.txt\n", argv[0]);
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
        int A = 0;
        std::string ts, mask;
        unsigned long r = 0;
        ls >> A >> ts >> r >> mask;
        float T = 0.0f;
        bool ok = !ls.fail() && A >= 1 && A <= 32 && hex_float(ts, &T) && mask.size() == (size_t)A;
        // every array has exactly the size the header documents: an access past it is the sanitizer's to find
        std::vector<float> p, pi;
        std::vector<uint8_t> legal;
        if (ok) {
            for (char c : mask) {
                ok = ok && (c == '0' || c == '1');
                legal.push_back(c == '1');
            }
            for (int a = 0; a < A && ok; ++a) {
                std::string ps;
                float x = 0.0f;
                ls >> ps;
                ok = !ls.fail() && hex_float(ps, &x);
                p.push_back(x);
            }
            std::string rest;
            if (ok && (ls >> rest)) ok = false;
        }
        int action = -1;
        if (ok) {
            pi.assign((size_t)A, -1.0f);
            action = mzp_row(p.data(), legal.data(), A, T, (uint32_t)r, pi.data());
        }
        if (action < 0) {
            std::cout << "rejected\n";
            continue;
        }
        std::cout << action;
        for (int a = 0; a < A; ++a) {
            uint32_t b;
            std::memcpy(&b, &pi[(size_t)a], 4);
            char buf[16];
            std::snprintf(buf, sizeof(buf), " %08x", b);
            std::cout << buf;
        }
        std::cout << "\n";
    }
    std::fprintf(stderr, "%ld rows\n", n);
    return 0;
}
