// gd_flow_cli.hpp -- what gd_particle_flow and gd_grid_flow share: the command line of the reference's
// analyze_particle_flow / analyze_grid_flow (__main__.py), the stored config JSON as Python's json.dumps prints it and its
// SHA-256 name (analysis.py: run), the input history (load_positions), and the HDF5 datasets of the output file
// (put_dataset with h5py's filters).  The computation itself is libgdyn's (include/gdyn_flow.h).
#pragma once
#include <hdf5.h>

#include <algorithm>
#include <array>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_flow.h"
#include "gd_cli_util.hpp"
#include "gd_h5util.hpp"

namespace gd {
namespace flow {

struct options {
    std::string name;                 // empty: sha256(config)[:7]
    bool has_smoothing = false;
    long smoothing = 0;
    long delay = 1;
    bool has_radius = false;
    double radius = 0;
    bool has_interval = false;
    double interval = 0;
    std::array<double, 2> range[3] = {};
    bool has_range[3] = {false, false, false};
    bool dry_run = false;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

// argparse's conventions: "--opt value" or "--opt=value"; exit status 2 with a usage line on any error
inline int parse(int argc, char **argv, bool grid, options &o, std::string &err)
{
    std::vector<std::string> pos;
    for (int k = 1; k < argc; k++) {
        std::string a = argv[k], v;
        if (a.size() > 2 && a.compare(0, 2, "--") == 0) {
            if (a == "--dry-run") { o.dry_run = true; continue; }
            auto eq = a.find('=');
            bool const inline_value = eq != std::string::npos;
            std::string const key = inline_value ? a.substr(0, eq) : a;
            if (inline_value) v = a.substr(eq + 1);
            else if (k + 1 < argc) v = argv[++k];
            else { err = "argument " + key + ": expected one argument"; return 2; }
            bool ok = true;
            if (key == "--name") o.name = v;
            else if (key == "--smoothing") ok = o.has_smoothing = cli::parse_int(v, o.smoothing);
            else if (key == "--velocity-delay") ok = cli::parse_int(v, o.delay);
            else if (key == "--scan-radius") ok = o.has_radius = cli::parse_float(v, o.radius);
            else if (key == "--jobs") { long j; ok = cli::parse_int(v, j); }      // accepted; one device does the work
            else if (grid && key == "--grid-interval") ok = o.has_interval = cli::parse_float(v, o.interval);
            else if (grid && (key == "--x-range" || key == "--y-range" || key == "--z-range")) {
                int const axis = key[2] - 'x';
                auto comma = v.find(',');
                ok = comma != std::string::npos && v.find(',', comma + 1) == std::string::npos &&
                     cli::parse_float(v.substr(0, comma), o.range[axis][0]) && cli::parse_float(v.substr(comma + 1), o.range[axis][1]);
                o.has_range[axis] = ok;
            } else { err = "unrecognized arguments: " + a; return 2; }
            if (!ok) { err = "argument " + key + ": invalid value: '" + v + "'"; return 2; }
        } else {
            pos.push_back(a);
        }
    }
    if (!o.has_radius) { err = "the following arguments are required: --scan-radius"; return 2; }
    if (grid && (!o.has_interval || !o.has_range[0] || !o.has_range[1] || !o.has_range[2])) {
        err = "the following arguments are required: --grid-interval, --x-range, --y-range, --z-range";
        return 2;
    }
    if (o.dry_run && pos.empty()) return 0;
    if (pos.size() < 2) { err = "the following arguments are required: outfile, trajfiles"; return 2; }
    o.outfile = pos[0];
    o.trajfiles.assign(pos.begin() + 1, pos.end());
    return 0;
}

inline std::string config_json(options const &o, bool grid)
{
    std::ostringstream s;
    s << "{\"smoothing\": " << (o.has_smoothing ? std::to_string(o.smoothing) : "null") << ", \"velocity_delay\": " << o.delay
      << ", \"scan_radius\": " << cli::py_float(o.radius);
    if (grid) {
        s << ", \"grid_interval\": " << cli::py_float(o.interval);
        char const *names[3] = {"x_range", "y_range", "z_range"};
        for (int a = 0; a < 3; a++) s << ", \"" << names[a] << "\": [" << cli::py_float(o.range[a][0]) << ", " << cli::py_float(o.range[a][1]) << "]";
    }
    s << "}";
    return s.str();
}

// FIPS 180-4 SHA-256
inline std::string sha256_hex(std::string const &msg)
{
    static const uint32_t K[64] = {
        0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
        0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
        0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
        0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
        0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
        0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    auto rotr = [](uint32_t x, int n) { return (x >> n) | (x << (32 - n)); };
    std::vector<unsigned char> m(msg.begin(), msg.end());
    uint64_t const bits = (uint64_t)m.size() * 8;
    m.push_back(0x80);
    while (m.size() % 64 != 56) m.push_back(0);
    for (int k = 7; k >= 0; k--) m.push_back((unsigned char)(bits >> (8 * k)));
    for (std::size_t blk = 0; blk < m.size(); blk += 64) {
        uint32_t w[64];
        for (int t = 0; t < 16; t++)
            w[t] = (uint32_t)m[blk + 4 * t] << 24 | (uint32_t)m[blk + 4 * t + 1] << 16 | (uint32_t)m[blk + 4 * t + 2] << 8 | m[blk + 4 * t + 3];
        for (int t = 16; t < 64; t++) {
            uint32_t const s0 = rotr(w[t - 15], 7) ^ rotr(w[t - 15], 18) ^ (w[t - 15] >> 3);
            uint32_t const s1 = rotr(w[t - 2], 17) ^ rotr(w[t - 2], 19) ^ (w[t - 2] >> 10);
            w[t] = w[t - 16] + s0 + w[t - 7] + s1;
        }
        uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
        for (int t = 0; t < 64; t++) {
            uint32_t const t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[t] + w[t];
            uint32_t const t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
            hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
        }
        h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
    }
    char out[65];
    for (int k = 0; k < 8; k++) std::snprintf(out + 8 * k, 9, "%08x", h[k]);
    return std::string(out, 64);
}

inline std::string analysis_name(options const &o, std::string const &config) { return o.name.empty() ? sha256_hex(config).substr(0, 7) : o.name; }

// load_positions: /snapshots/interphase/<step>/positions for the steps of .steps in stored order, as float32 (F, N, 3)
inline std::vector<float> load_history(std::string const &path, uint32_t &frames, uint32_t &beads)
{
    h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    h5::check(file >= 0, "cannot open " + path);
    h5::hid phase(H5Gopen2(file, "/snapshots/interphase", H5P_DEFAULT));
    h5::check(phase >= 0, path + ": no /snapshots/interphase");
    auto const steps = h5::read_string_list(phase, ".steps");
    h5::check(!steps.empty(), path + ": no interphase snapshots");
    std::vector<float> out;
    std::size_t n0 = 0;
    for (auto const &s : steps) {
        h5::hid snap(H5Gopen2(phase, s.c_str(), H5P_DEFAULT));
        h5::check(snap >= 0, path + ": missing snapshot " + s);
        std::size_t n = 0;
        auto x = h5::read_array<float>(snap, "positions", 3, H5T_NATIVE_FLOAT, &n);
        if (out.empty()) n0 = n;
        h5::check(n == n0 && n > 0, path + ": snapshots disagree on the number of beads");
        out.insert(out.end(), x.begin(), x.end());
    }
    frames = (uint32_t)steps.size();
    beads = (uint32_t)n0;
    return out;
}

struct device {      // one gd_flow handle; every failure of the library ends the program with its message
    gd_flow *h = nullptr;
    device()
    {
        gd_flow_desc d{0, 0};
        cli::check(gd_flow_create(&d, &h));
    }
    ~device() { gd_flow_destroy(h); }
};

// common front: parse, print the config for --dry-run; returns -1 to go on, else the exit status
inline int front(int argc, char **argv, bool grid, options &o, std::string &config, std::string &name)
{
    std::string err;
    char const *prog = grid ? "gd_grid_flow" : "gd_particle_flow";
    if (parse(argc, argv, grid, o, err)) {
        std::fprintf(stderr, "usage: %s [--name NAME] [--smoothing W] [--velocity-delay D] --scan-radius R%s [--jobs J] [--dry-run] outfile trajfiles ...\n"
                             "%s: error: %s\n",
                     prog, grid ? " --grid-interval H --x-range A,B --y-range A,B --z-range A,B" : "", prog, err.c_str());
        return 2;
    }
    config = config_json(o, grid);
    name = analysis_name(o, config);
    if (o.dry_run) {
        std::printf("%s\n%s\n", config.c_str(), name.c_str());
        return 0;
    }
    if (o.delay < 0 || o.smoothing < 0) {
        std::fprintf(stderr, "%s: error: --velocity-delay and --smoothing must be >= 0\n", prog);
        return 2;
    }
    return -1;
}

}  // namespace flow
}  // namespace gd
