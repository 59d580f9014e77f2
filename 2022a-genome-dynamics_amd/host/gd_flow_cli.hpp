// gd_flow_cli.hpp -- what gd_particle_flow and gd_grid_flow share: the command line of the reference's
// analyze_particle_flow / analyze_grid_flow (__main__.py), the stored config JSON as Python's json.dumps prints it and its
// SHA-256 name (analysis.py: run), the input history (load_positions), the grid mesh, and the writers of the two output layouts
// (cli::put with h5py's filters).  The computation itself is libgdyn's (include/gdyn_flow.h).  gd_interphase writes the same
// outputs from frames recorded on the device (--particle-flow / --grid-flow) through the same writers.
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

// the positionals "outfile trajfiles ..." of a trajectory analysis; --dry-run alone is served without them.  0 or 2 with a message
inline int take_files(std::vector<std::string> const &pos, bool dry_run, std::string &outfile, std::vector<std::string> &trajfiles, std::string &err)
{
    if (dry_run && pos.empty()) return 0;
    if (pos.size() < 2) { err = "the following arguments are required: outfile, trajfiles"; return 2; }
    outfile = pos[0];
    trajfiles.assign(pos.begin() + 1, pos.end());
    return 0;
}

// argparse's conventions: "--opt value" or "--opt=value"; exit status 2 with a usage line on any error.  grid_options: the grid's
// options are accepted (a particle analysis that shares its command line with a grid analysis ignores them)
inline int parse(int argc, char **argv, bool grid, options &o, std::string &err, bool grid_options)
{
    using cli::kind;
    static cli::table const particle = {{"--dry-run", kind::flag}, {"--name", kind::value}, {"--smoothing", kind::value}, {"--velocity-delay", kind::value},
                                        {"--scan-radius", kind::value}, {"--jobs", kind::value}};
    static cli::table const with_grid = [] {
        cli::table t = particle;
        for (char const *key : {"--grid-interval", "--x-range", "--y-range", "--z-range"}) t.push_back({key, kind::value});
        return t;
    }();
    std::vector<std::string> pos;
    err = cli::scan(argc, argv, grid_options ? with_grid : particle, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--name") return o.name = v, std::string();
        if (key == "--smoothing") return cli::valid_if(o.has_smoothing = cli::parse_int(v, o.smoothing), v);
        if (key == "--velocity-delay") return cli::to_int(v, o.delay);
        if (key == "--scan-radius") return cli::valid_if(o.has_radius = cli::parse_float(v, o.radius), v);
        if (key == "--jobs") { long j; return cli::to_int(v, j); }      // accepted; one device does the work
        if (key == "--grid-interval") return cli::valid_if(o.has_interval = cli::parse_float(v, o.interval), v);
        int const axis = key[2] - 'x';      // --x-range, --y-range, --z-range
        auto const comma = v.find(',');
        o.has_range[axis] = comma != std::string::npos && v.find(',', comma + 1) == std::string::npos &&
                            cli::parse_float(v.substr(0, comma), o.range[axis][0]) && cli::parse_float(v.substr(comma + 1), o.range[axis][1]);
        return cli::valid_if(o.has_range[axis], v);
    }, pos);
    if (!err.empty()) return 2;
    if (!o.has_radius) { err = "the following arguments are required: --scan-radius"; return 2; }
    if (grid && (!o.has_interval || !o.has_range[0] || !o.has_range[1] || !o.has_range[2])) {
        err = "the following arguments are required: --grid-interval, --x-range, --y-range, --z-range";
        return 2;
    }
    return take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

inline int parse(int argc, char **argv, bool grid, options &o, std::string &err) { return parse(argc, argv, grid, o, err, grid); }

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

// load_positions: /snapshots/<phase>/<step>/positions for the steps of .steps in stored order, as float32 (F, N, 3)
inline std::vector<float> load_history(std::string const &path, uint32_t &frames, uint32_t &beads, std::string const &phase_name = "interphase")
{
    h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    h5::check(file >= 0, "cannot open " + path);
    h5::hid phase(H5Gopen2(file, ("/snapshots/" + phase_name).c_str(), H5P_DEFAULT));
    h5::check(phase >= 0, path + ": no /snapshots/" + phase_name);
    auto const steps = h5::read_string_list(phase, ".steps");
    h5::check(!steps.empty(), path + ": no " + phase_name + " snapshots");
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

using device = cli::handle<gd_flow, gd_flow_destroy>;      // one gd_flow handle

inline void open(device &dev, int ordinal = 0)
{
    dev.open([ordinal](gd_flow **h) { gd_flow_desc const d{ordinal, 0}; return gd_flow_create(&d, h); });
}

inline bool smoothed(options const &o) { return o.has_smoothing && o.smoothing > 0; }

// the main of both programs: parse, print the config for --dry-run, else body(o, config, name, prog) is the analysis
template <typename Body>
int main(int argc, char **argv, bool grid, Body &&body)
{
    std::string const prog = grid ? "gd_grid_flow" : "gd_particle_flow";
    std::string const usage = "usage: " + prog + " [--name NAME] [--smoothing W] [--velocity-delay D] --scan-radius R" +
                              (grid ? " --grid-interval H --x-range A,B --y-range A,B --z-range A,B" : "") + " [--jobs J] [--dry-run] outfile trajfiles ...\n";
    options o;
    return cli::run(usage, prog.c_str(), (prog + ": error:").c_str(), [&](std::string &err) { return parse(argc, argv, grid, o, err); }, cli::no_plan, [&] {
        std::string const config = config_json(o, grid), name = analysis_name(o, config);
        if (o.dry_run) {
            std::printf("%s\n%s\n", config.c_str(), name.c_str());
            return 0;
        }
        if (o.delay < 0 || o.smoothing < 0) {
            std::fprintf(stderr, "%s: error: --velocity-delay and --smoothing must be >= 0\n", prog.c_str());
            return 2;
        }
        body(o, config, name, prog.c_str());
        return 0;
    });
}

// ---- /particle_flow/<name> of the output file: .config, <sample>/{position,velocity}, and at the end .samples
class particle_writer {
public:
    particle_writer(std::string const &outfile, std::string const &name, std::string const &config)
        : _file(cli::open_output(outfile)), _group(cli::require_group(_file, "/particle_flow/" + name))
    {
        h5::write_string(_group, ".config", config);
    }
    // position: the smoothed fp64 history when given, else the float32 history itself
    void put(std::string const &sample, uint32_t F, uint32_t N, float const *history, double const *smoothed_history, float const *flows)
    {
        _samples.push_back(sample);
        cli::filters const f;
        std::vector<hsize_t> const dims = {F, N, 3};
        if (smoothed_history) cli::put(_group, sample + "/position", smoothed_history, dims, &f);
        else cli::put(_group, sample + "/position", history, dims, &f);
        cli::put(_group, sample + "/velocity", flows, dims, &f);
    }
    void finish() { h5::write_fixed_string_list(_group, ".samples", _samples); }      // this run's samples only, as the reference does

private:
    h5::hid _file, _group;
    std::vector<std::string> _samples;
};

inline std::vector<double> arange(double start, double stop, double step)      // numpy.arange for floats, its fill rule included
{
    double const len = std::ceil((stop - start) / step);
    std::vector<double> out(len > 0 ? (std::size_t)len : 0);
    if (out.empty()) return out;
    out[0] = start;
    if (out.size() > 1) out[1] = start + step;
    double const delta = (start + step) - start;
    for (std::size_t i = 2; i < out.size(); i++) out[i] = start + (double)i * delta;
    return out;
}

struct mesh {      // analyze_grid_flow's grid: inclusive aranges, points in np.meshgrid(x, y, z) ('xy') order
    std::size_t G = 0;
    std::vector<double> points;
    std::vector<int64_t> indices;
    int64_t shape[3] = {0, 0, 0};

    explicit mesh(options const &o)
    {
        if (!(o.interval > 0)) throw std::runtime_error("--grid-interval must be positive");
        std::vector<double> axes[3];
        for (int a = 0; a < 3; a++) axes[a] = arange(o.range[a][0], o.range[a][1] + o.interval * 0.1, o.interval);
        std::size_t const nx = axes[0].size(), ny = axes[1].size(), nz = axes[2].size();
        G = nx * ny * nz;
        if (G == 0 || G > (1u << 28)) throw std::runtime_error("the grid has " + std::to_string(G) + " points");
        points.resize(3 * G);
        indices.resize(3 * G);
        for (std::size_t iy = 0, k = 0; iy < ny; iy++)      // y slowest, then x, then z
            for (std::size_t ix = 0; ix < nx; ix++)
                for (std::size_t iz = 0; iz < nz; iz++, k++) {
                    points[3 * k] = axes[0][ix]; points[3 * k + 1] = axes[1][iy]; points[3 * k + 2] = axes[2][iz];
                    indices[3 * k] = (int64_t)ix; indices[3 * k + 1] = (int64_t)iy; indices[3 * k + 2] = (int64_t)iz;
                }
        shape[0] = (int64_t)nx; shape[1] = (int64_t)ny; shape[2] = (int64_t)nz;
    }
};

// estimate_scaleoffset_factor(values, q=1): -floor(log10(0.1 * percentile(values[values > 0], 1))) in float32, numpy's linear rule
inline int scaleoffset_factor(std::vector<float> const &v)
{
    std::vector<float> pos;
    for (float x : v) if (x > 0) pos.push_back(x);
    if (pos.empty()) throw std::runtime_error("no positive flow component: the scale-offset factor is undefined");
    std::sort(pos.begin(), pos.end());
    double const idx = 0.01 * (double)(pos.size() - 1);
    std::size_t const lo = (std::size_t)std::floor(idx);
    std::size_t const hi = std::min(lo + 1, pos.size() - 1);
    float const t = (float)(idx - (double)lo), a = pos[lo], b = pos[hi], diff = b - a;
    float const p = t >= 0.5f ? b - diff * (1.0f - t) : a + diff * t;
    float const resolution = 0.1f * p;
    return -(int)std::floor(std::log10(resolution));
}

inline std::vector<std::string> remove_duplicates(std::vector<std::string> const &xs)      // keeps the last occurrence
{
    std::vector<std::string> out;
    for (std::size_t i = 0; i < xs.size(); i++)
        if (std::find(xs.begin() + (long)i + 1, xs.end(), xs[i]) == xs.end()) out.push_back(xs[i]);
    return out;
}

// ---- /grid_flow/<name> of the output file: .config, .grid/{shape,points,indices}, <sample>/{flows,coverages}, and at the end
// .samples merged with those of earlier runs
class grid_writer {
public:
    grid_writer(std::string const &outfile, std::string const &name, std::string const &config, mesh const &m)
        : _file(cli::open_output(outfile)), _group(cli::require_group(_file, "/grid_flow/" + name)), _G(m.G)
    {
        h5::write_string(_group, ".config", config);
        _samples = h5::read_string_list(_group, ".samples");      // incremental analysis: earlier samples stay listed
        cli::put(_group, ".grid/shape", m.shape, {3}, nullptr);
        cli::put(_group, ".grid/points", m.points.data(), {m.G, 3}, nullptr);
        cli::put(_group, ".grid/indices", m.indices.data(), {m.G, 3}, nullptr);
    }
    void put(std::string const &sample, uint32_t F, std::vector<float> const &flows, std::vector<int32_t> const &coverages, int factor)
    {
        _samples.push_back(sample);
        cli::filters ff;
        ff.scaleoffset_kind = H5Z_SO_FLOAT_DSCALE;
        ff.scaleoffset_factor = factor;
        cli::put(_group, sample + "/flows", flows.data(), {F, _G, 3}, &ff);
        cli::filters fc;
        fc.scaleoffset_kind = H5Z_SO_INT;
        fc.scaleoffset_factor = H5Z_SO_INT_MINBITS_DEFAULT;
        cli::put(_group, sample + "/coverages", coverages.data(), {F, _G}, &fc);
        H5Fflush(_file, H5F_SCOPE_GLOBAL);
    }
    void finish() { h5::write_fixed_string_list(_group, ".samples", remove_duplicates(_samples)); }

private:
    h5::hid _file, _group;
    std::size_t _G;
    std::vector<std::string> _samples;
};

}  // namespace flow
}  // namespace gd
