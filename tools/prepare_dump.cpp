// What prepare() makes of a list of configurations, written out so that two trees can be compared byte for byte (profiles/prepare_stages):
// a program of its own, host code only.  It uses prepare() and the members of Prepared that the consumers read, nothing else of the header.
//
// Build: g++ -O2 -std=c++17 -I sponge_amd/csrc tools/prepare_dump.cpp -o prepare_dump        (-I <another tree>/sponge_amd/csrc: that tree's)
// usage: prepare_dump CONFIGS OUTDIR               per configuration k of the file tools/prepare_configs.py writes: OUTDIR/k.bin = the words of
//                                                  Prepared::consts, OUTDIR/k.txt = return code, message, flags, offsets and the field block
//        prepare_dump --time CONFIGS [NAME ...]    median of 20 calls of prepare() alone, milliseconds, for the named configurations
//                                                  (default: bls_t3_a5_8_31 and bls_t9_a5_8_57)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "pmx_prepare.hpp"

using namespace pmx;

struct Config {
    std::string name;
    pmx_config cfg;
    std::vector<uint64_t> ark, mds;   // four words per constant
};

static bool hex_words(const std::string &tok, uint64_t out[4]) {   // up to 64 hex digits, little-endian words
    if (tok.empty() || tok.size() > 64) return false;
    out[0] = out[1] = out[2] = out[3] = 0;
    for (size_t i = 0; i < tok.size(); ++i) {
        const char ch = tok[tok.size() - 1 - i];
        const int d = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
        if (d < 0) return false;
        out[i / 16] |= (uint64_t)d << (4 * (i % 16));
    }
    return true;
}

static bool read_configs(const char *path, std::vector<Config> &all) {
    std::ifstream in(path);
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream ls(line);
        Config c;
        std::string tok;
        uint64_t v[6][4], w[4];
        if (!(ls >> c.name)) continue;
        if (!(ls >> tok) || !hex_words(tok, c.cfg.modulus)) return false;
        for (int i = 1; i < 6; ++i)
            if (!(ls >> tok) || !hex_words(tok, v[i])) return false;
        c.cfg.rate = (uint32_t)v[1][0];
        c.cfg.capacity = (uint32_t)v[2][0];
        c.cfg.alpha = v[3][0];
        c.cfg.full_rounds = (uint32_t)v[4][0];
        c.cfg.partial_rounds = (uint32_t)v[5][0];
        const size_t t = (size_t)c.cfg.rate + c.cfg.capacity, n_ark = ((size_t)c.cfg.full_rounds + c.cfg.partial_rounds) * t;
        while (ls >> tok) {
            if (!hex_words(tok, w)) return false;
            std::vector<uint64_t> &dst = c.ark.size() < 4 * n_ark ? c.ark : c.mds;
            dst.insert(dst.end(), w, w + 4);
        }
        if (c.ark.size() != 4 * n_ark || c.mds.size() != 4 * t * t) return false;
        c.ark.push_back(0);   // (never empty: prepare() is handed pointers)
        c.mds.push_back(0);
        all.push_back(std::move(c));
    }
    for (Config &c : all) {
        c.cfg.ark = c.ark.data();
        c.cfg.mds = c.mds.data();
    }
    return !all.empty();
}

static void words(FILE *f, const char *name, const uint32_t *w, size_t n) {
    std::fprintf(f, "%s", name);
    for (size_t i = 0; i < n; ++i) std::fprintf(f, " %08x", w[i]);
    std::fprintf(f, "\n");
}

static int dump(const std::vector<Config> &all, const std::string &dir) {
    for (size_t k = 0; k < all.size(); ++k) {
        Prepared pp;
        std::string err;
        const int rc = prepare(&all[k].cfg, pp, err);
        FILE *txt = std::fopen((dir + "/" + std::to_string(k) + ".txt").c_str(), "w");
        FILE *bin = std::fopen((dir + "/" + std::to_string(k) + ".bin").c_str(), "wb");
        if (!txt || !bin) return 2;
        std::fprintf(txt, "name %s\nrc %d\nerr %s\n", all[k].name.c_str(), rc, err.c_str());
        if (rc == PMX_OK) {   // (a refused configuration leaves the rest unset)
            std::fprintf(txt, "has_opt %d\nmfma_dense %d\nmfma_window %u\nunit_low_limb %d\nt %u\n", (int)pp.has_opt, (int)pp.mfma_dense, pp.mfma_window,
                         (int)pp.unit_low_limb, pp.t);
            std::fprintf(txt, "mds_offset %zu\nopt_offset %zu\ncoop_offset %zu\nmfma_offset %zu\nwin_offset %zu\nio_offset %zu\nwords %zu\n", pp.mds_offset,
                         pp.opt_offset, pp.coop_offset, pp.mfma_offset, pp.win_offset, pp.io_offset, pp.consts.size());
            words(txt, "f.p", pp.f.p, kN);
            std::fprintf(txt, "f.pinv %08x\nf.unit %u\nf.io %td\n", pp.f.pinv, pp.f.unit, pp.f.io - pp.consts.data());
            words(txt, "one", pp.one.l, kN);
            std::fprintf(txt, "c %u %u %u %u %u %llx\n", pp.c.rate, pp.c.capacity, pp.c.half_full, pp.c.partial_rounds, pp.c.total_rounds,
                         (unsigned long long)pp.c.alpha);
            if (!pp.consts.empty() && std::fwrite(pp.consts.data(), 4, pp.consts.size(), bin) != pp.consts.size()) return 2;
        }
        std::fclose(txt);
        std::fclose(bin);
    }
    std::printf("%zu configurations\n", all.size());
    return 0;
}

static int time_prepare(const std::vector<Config> &all, std::vector<std::string> names) {
    if (names.empty()) names = {"bls_t3_a5_8_31", "bls_t9_a5_8_57"};
    for (const std::string &name : names) {
        const Config *c = nullptr;
        for (const Config &x : all)
            if (x.name == name) c = &x;
        if (!c) {
            std::fprintf(stderr, "no configuration named %s\n", name.c_str());
            return 2;
        }
        std::vector<double> ms;
        for (int i = 0; i < 20; ++i) {
            Prepared pp;
            std::string err;
            const auto t0 = std::chrono::steady_clock::now();
            const int rc = prepare(&c->cfg, pp, err);
            const auto t1 = std::chrono::steady_clock::now();
            if (rc != PMX_OK) return 2;
            ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
        }
        std::sort(ms.begin(), ms.end());
        std::printf("%s  median of 20: %.3f ms  (min %.3f, max %.3f)\n", name.c_str(), (ms[9] + ms[10]) / 2, ms.front(), ms.back());
    }
    return 0;
}

int main(int argc, char **argv) {
    const bool timing = argc >= 2 && std::string(argv[1]) == "--time";
    if (argc < 3) {
        std::fprintf(stderr, "usage: prepare_dump CONFIGS OUTDIR | prepare_dump --time CONFIGS [NAME ...]\n");
        return 2;
    }
    std::vector<Config> all;
    if (!read_configs(argv[timing ? 2 : 1], all)) {
        std::fprintf(stderr, "cannot read the configurations\n");
        return 2;
    }
    return timing ? time_prepare(all, std::vector<std::string>(argv + 3, argv + argc)) : dump(all, argv[2]);
}
