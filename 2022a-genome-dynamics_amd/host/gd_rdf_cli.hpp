// gd_rdf_cli.hpp -- what gd_rdf_analysis and gd_rdf_analysis_hetero share: the command lines of the reference's
// 4-sim-ab/box/src/rdf_analysis/main.cc and rdf_analysis_hetero/main.cc, the inputs of their analysis.cc (A/B factors, box
// size, snapshot keys, positions), the bin volumes and weights of distance_histogram.cc and the stdout format.  The pair
// counts are libgdyn's (include/gdyn_rdf.h).
#pragma once
#include <hdf5.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include <json.hpp>   // nlohmann/json single header

#include "../../include/gdyn.h"
#include "../../include/gdyn_rdf.h"
#include "gd_cli_util.hpp"
#include "gd_h5util.hpp"

namespace gd {
namespace rdf {

constexpr double PI = 3.1416;      // distance_histogram.cc:12 -- the reference's value, not pi

struct options {
    bool hetero = false;
    std::string type;                 // rdf_analysis: "" = all; hetero: centre type, default "A" (main.cc:20)
    bool has_steps = false;
    long step_start = 0, step_end = 0;    // parsed and checked, then ignored, as in the reference (analysis.cc:68)
    double bin_width = 0.1, max_distance = 1;      // analysis.hpp defaults
    bool dry_run = false;
    std::string file;
};

inline const char *usage(bool hetero)
{
    return hetero ? "usage:\n"
                    "  gd_rdf_analysis_hetero [options] <FILE>\n"
                    "\n"
                    "  <FILE>  HDF5 trajectory file to analyze\n"
                    "\n"
                    "options:\n"
                    "  --type <TYPE>          Type of center particles used in RDF analysis [default: A]\n"
                    "  --bin-width <DIST>     Bin width\n"
                    "  --max-distance <DIST>  Max distance for analysis\n"
                    "  --dry-run              Print the derived setup and exit without touching the GPU\n"
                    "  -h, --help             Print this help message and exit\n"
                  : "usage:\n"
                    "  gd_rdf_analysis [options] <FILE>\n"
                    "\n"
                    "  <FILE>  HDF5 trajectory file to analyze\n"
                    "\n"
                    "options:\n"
                    "  --type <TYPE>          Particle type to select\n"
                    "  --steps <RANGE>        Step or range of steps (start:end) to analyze\n"
                    "  --bin-width <DIST>     Bin width\n"
                    "  --max-distance <DIST>  Max distance for analysis\n"
                    "  --dry-run              Print the derived setup and exit without touching the GPU\n"
                    "  -h, --help             Print this help message and exit\n";
}

// std::stod / std::stol as the reference calls them: leading blanks skipped, a prefix parsed, the rest ignored
inline bool prefix_double(std::string const &s, double &out)
{
    char *end = nullptr;
    errno = 0;
    out = std::strtod(s.c_str(), &end);
    return end != s.c_str() && errno != ERANGE;
}

inline bool prefix_long(std::string const &s, long &out, std::size_t &pos)
{
    char *end = nullptr;
    errno = 0;
    out = std::strtol(s.c_str(), &end, 10);
    pos = (std::size_t)(end - s.c_str());
    return end != s.c_str() && errno != ERANGE;
}

// main.cc:84-102 parse_range: "start" or "start:end"
inline void parse_range(std::string const &arg, long &start, long &end)
{
    std::size_t pos = 0, pos2 = 0;
    if (!prefix_long(arg, start, pos)) throw std::invalid_argument("invalid range specification: '" + arg + "'");
    end = start;
    if (pos < arg.size()) {
        if (arg[pos] != ':' || !prefix_long(arg.substr(pos + 1), end, pos2))
            throw std::invalid_argument("invalid range specification: '" + arg + "'");
    }
}

inline double parse_distance(std::string const &arg)      // main.cc:105-109
{
    double v;
    if (!prefix_double(arg, v)) throw std::invalid_argument("invalid distance: '" + arg + "'");
    return v;
}

// docopt's conventions for the reference's usage: "--opt value" or "--opt=value", one <FILE>.  Returns 0 (go on), 1 (help
// printed) or 2 (usage error); value errors throw std::invalid_argument, as std::stod / parse_range do in the reference.
inline int parse(int argc, char **argv, options &o, std::string &err)
{
    std::vector<std::string> files;
    std::string steps, bin_width, max_distance;
    bool has_bin_width = false, has_max_distance = false;
    if (o.hetero) o.type = "A";
    for (int k = 1; k < argc; k++) {
        std::string const a = argv[k];
        if (a == "-h" || a == "--help") return 1;
        if (a == "--dry-run") { o.dry_run = true; continue; }
        if (a.size() > 1 && a[0] == '-') {
            auto const eq = a.find('=');
            std::string const key = eq == std::string::npos ? a : a.substr(0, eq);
            bool const known = key == "--type" || key == "--bin-width" || key == "--max-distance" || (!o.hetero && key == "--steps");
            if (!known) { err = key + " is not recognized"; return 2; }
            std::string v;
            if (eq != std::string::npos) v = a.substr(eq + 1);
            else if (k + 1 < argc) v = argv[++k];
            else { err = key + " requires argument"; return 2; }
            if (key == "--type") o.type = v;
            else if (key == "--steps") { o.has_steps = true; steps = v; }
            else if (key == "--bin-width") { has_bin_width = true; bin_width = v; }
            else { has_max_distance = true; max_distance = v; }
        } else {
            files.push_back(a);
        }
    }
    if (files.size() != 1) { err = files.empty() ? "<FILE> is missing" : "unexpected argument " + files[1]; return 2; }
    o.file = files[0];
    // converted after the whole line was accepted, in the order of main.cc:62-78
    if (o.has_steps) parse_range(steps, o.step_start, o.step_end);
    if (has_bin_width) o.bin_width = parse_distance(bin_width);
    if (has_max_distance) o.max_distance = parse_distance(max_distance);
    return 0;
}

struct setup {
    std::size_t n_points = 0;
    std::vector<uint32_t> centers, targets;      // targets: cross mode only
    double box_size = 0, volume = 0, expected_density = 0, unit_weight = 0;
    uint32_t n_bins = 0;
    std::vector<double> bin_volumes;
    std::vector<std::string> keys;
};

// distance_histogram.cc:16-37: bin i spans [w i, w (i + 1)] clipped at max_distance; volume 4 PI / 3 (r_max^3 - r_min^3)
inline std::vector<double> bin_volumes(double bin_width, double max_distance, uint32_t n_bins)
{
    std::vector<double> v;
    for (uint32_t i = 0; i < n_bins; i++) {
        double const r_min = bin_width * double(i);
        double r_max = bin_width * double(i + 1);
        if (r_max > max_distance) r_max = max_distance;
        double const dr3 = r_max * r_max * r_max - r_min * r_min * r_min;
        v.push_back(4 * PI / 3 * dr3);
    }
    return v;
}

// analysis.cc of either program up to its frame loop
inline setup prepare(options const &o, hid_t file)
{
    setup s;
    std::size_t rows = 0;
    auto const ab = h5::read_array<double>(file, "metadata/ab_factors", 2, H5T_NATIVE_DOUBLE, &rows);      // float32, widened
    s.n_points = rows;
    if (o.hetero) {      // rdf_analysis_hetero/analysis.cc:32-54
        double center_a = -1;
        if (o.type == "A") center_a = 1;
        if (o.type == "B") center_a = 0;
        if (center_a == -1) throw std::runtime_error("invalid center type: '" + o.type + "'");
        for (std::size_t i = 0; i < rows; i++) (std::fabs(ab[2 * i] - center_a) < 1e-6 ? s.centers : s.targets).push_back((uint32_t)i);
    } else {             // rdf_analysis/analysis.cc:31-52: anything but A or B selects every bead
        double a_factor = -1;
        if (o.type == "A") a_factor = 1;
        if (o.type == "B") a_factor = 0;
        for (std::size_t i = 0; i < rows; i++)
            if (a_factor == -1 || std::fabs(ab[2 * i] - a_factor) < 0.1) s.centers.push_back((uint32_t)i);
    }
    auto const config = nlohmann::json::parse(h5::read_string(file, "metadata/config"));
    auto const it = config.find("box_size");
    if (it == config.end() || !it->is_number()) throw std::runtime_error("metadata/config has no numeric box_size");
    s.box_size = it->get<double>();
    s.volume = s.box_size * s.box_size * s.box_size;
    double const n_norm = double(o.hetero ? s.targets.size() : s.centers.size());      // the density the RDF is normalised to
    s.expected_density = n_norm / s.volume;
    s.unit_weight = o.hetero ? 1 / double(s.centers.size()) : 2 / double(s.centers.size());      // distance_histogram.cc:44 / :47
    s.n_bins = gd_rdf_bins(o.bin_width, o.max_distance);
    if (!s.n_bins)
        throw std::runtime_error("--bin-width and --max-distance must be positive and finite, with at most " + std::to_string(GD_RDF_MAX_BINS) +
                                 " bins");
    if (!(s.box_size > 0) || !std::isfinite(s.box_size)) throw std::runtime_error("box_size must be positive and finite");
    s.bin_volumes = bin_volumes(o.bin_width, o.max_distance, s.n_bins);
    h5::hid snaps(H5Gopen2(file, "snapshots", H5P_DEFAULT));
    h5::check(snaps >= 0, "missing group snapshots");
    h5::check(h5::exists(snaps, ".steps"), "missing dataset snapshots/.steps");
    s.keys = h5::read_string_list(snaps, ".steps");
    return s;
}

inline void print_setup(options const &o, setup const &s)
{
    std::printf("mode\t%s\n", o.hetero ? "cross" : "self");
    std::printf("n_points\t%zu\nn_center\t%zu\nn_target\t%zu\n", s.n_points, s.centers.size(), s.targets.size());
    std::printf("box_size\t%.17g\nbin_width\t%.17g\nmax_distance\t%.17g\nn_bins\t%u\n", s.box_size, o.bin_width, o.max_distance, s.n_bins);
    std::printf("expected_density\t%.17g\nunit_weight\t%.17g\nbin_volumes", s.expected_density, s.unit_weight);
    for (double v : s.bin_volumes) std::printf("\t%.17g", v);
    std::printf("\nframes\t%zu\nkeys", s.keys.size());
    for (auto const &k : s.keys) std::printf("\t%s", k.c_str());
    std::printf("\n");
}

// frames [k0, k1) of the snapshot keys as float32 (F, N, 3)
inline std::vector<float> read_frames(hid_t file, setup const &s, std::size_t k0, std::size_t k1)
{
    std::vector<float> out;
    out.reserve((k1 - k0) * s.n_points * 3);
    for (std::size_t k = k0; k < k1; k++) {
        std::size_t n = 0;
        auto const x = h5::read_array<float>(file, "snapshots/" + s.keys[k] + "/positions", 3, H5T_NATIVE_FLOAT, &n);
        h5::check(n == s.n_points, "snapshots/" + s.keys[k] + "/positions: " + std::to_string(n) + " rows, metadata/ab_factors has " +
                                       std::to_string(s.n_points));
        out.insert(out.end(), x.begin(), x.end());
    }
    return out;
}

// the frame loop of analysis.cc: counts on the device in batches (the next batch is read while the device counts), one line
// per frame of n_bins values count * unit_weight / bin_volume / expected_density, printed as std::ostream prints a double
inline void run(options const &o, hid_t file, setup const &s)
{
    std::size_t const F = s.keys.size();
    std::size_t const batch = std::max<std::size_t>(1, std::min<std::size_t>(4096, ((std::size_t)1 << 22) / std::max<std::size_t>(s.n_points, 1)));
    gd_rdf *h = nullptr;
    gd_rdf_desc const desc{0, (uint32_t)batch};
    cli::check(gd_rdf_create(&desc, &h));
    std::unique_ptr<gd_rdf, int (*)(gd_rdf *)> guard(h, gd_rdf_destroy);
    cli::check(gd_rdf_set_selection(h, (uint32_t)s.n_points, s.centers.data(), (uint32_t)s.centers.size(), o.hetero ? s.targets.data() : nullptr,
                               (uint32_t)s.targets.size()));
    double const box[3] = {s.box_size, s.box_size, s.box_size};
    std::vector<uint64_t> counts;
    std::future<std::vector<float>> next;
    if (F) next = std::async(std::launch::async, read_frames, file, std::cref(s), 0, std::min(batch, F));
    for (std::size_t k0 = 0; k0 < F; k0 += batch) {
        std::size_t const k1 = std::min(F, k0 + batch);
        std::vector<float> const xyz = next.get();      // HDF5 is called from one thread at a time: the reader, then nobody
        if (k1 < F) next = std::async(std::launch::async, read_frames, file, std::cref(s), k1, std::min(F, k1 + batch));
        counts.resize((k1 - k0) * s.n_bins);
        cli::check(gd_rdf_counts(h, xyz.data(), 0, (uint32_t)(k1 - k0), box, o.bin_width, o.max_distance, counts.data()));
        for (std::size_t f = 0; f < k1 - k0; f++) {
            for (uint32_t i = 0; i < s.n_bins; i++) {
                double const freq = double(counts[f * s.n_bins + i]) * s.unit_weight;
                double const density = freq / s.bin_volumes[i];
                if (i > 0) std::cout << '\t';
                std::cout << density / s.expected_density;
            }
            std::cout << '\n';
        }
    }
    std::cout.flush();
}

// main.cc of either program: status 0, 1 (error: <what>) or 2 (usage)
inline int main(int argc, char **argv, bool hetero)
{
    options o;
    o.hetero = hetero;
    std::string err;
    try {
        int const rc = parse(argc, argv, o, err);
        if (rc == 1) {
            std::fputs(usage(hetero), stdout);
            return 0;
        }
        if (rc == 2) {
            std::fprintf(stderr, "%s\n%s", err.c_str(), usage(hetero));
            return 2;
        }
        H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
        h5::hid file(H5Fopen(o.file.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
        h5::check(file >= 0, "cannot open " + o.file);
        setup const s = prepare(o, file);
        if (o.dry_run) print_setup(o, s);
        else run(o, file, s);
    } catch (std::exception const &e) {
        std::cout.flush();
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

}  // namespace rdf
}  // namespace gd
