// gd_hic_cli.hpp -- what gd_compute_interactions, gd_compute_local_alpha, gd_hic_power_law, gd_downsample and gd_hic_compartments share: the command
// lines of the reference's 2-signal/src/{compute_interactions, compute_local_alpha, downsample} and
// 5-sim-genome/scripts/hic_power_law, the reads of a multi-resolution cooler file (resolutions/<binsize>/bins/{chrom, start,
// end, <weights>} and pixels/{bin1_id, bin2_id, count}, the next chunk of pixels on a second thread while the device works) and
// their text outputs.  The sums and signals are libgdyn's (include/gdyn_hic.h).  gd_hic_compartments has no command in the
// reference: it is hic_analysis/cool.py (dense cis matrices, observed / expected, leading principal components) as a program with
// the conventions of its siblings.
//
// Deviations from the reference, all documented in DESIGN.md section 7e: sums over repeated pixels are true sums; a chromosome
// of 1 < n < 2 (W - 1) bins gets signals by the rule instead of an assertion; blacklisted names a file does not have are
// skipped; a name without a standard order, bins of one chromosome that are not contiguous and a missing weight column are
// errors before the pass.
#pragma once
#include <future>
#include <map>

#include "../../include/gdyn_hic.h"
#include "gd_cli_util.hpp"

namespace gd {
namespace hic {

enum class program { interactions, alpha, power_law, downsample, compartments };

inline const char *name_of(program p)
{
    switch (p) {
    case program::interactions: return "gd_compute_interactions";
    case program::alpha: return "gd_compute_local_alpha";
    case program::power_law: return "gd_hic_power_law";
    case program::compartments: return "gd_hic_compartments";
    default: return "gd_downsample";
    }
}

inline const char *usage(program p)
{
    switch (p) {
    case program::interactions: return "usage: gd_compute_interactions -b BINSIZE [-w BANDWIDTH] [-o OUT] [--dry-run] mcoolfile\n";
    case program::alpha: return "usage: gd_compute_local_alpha [-w WIDTH] [-b BINSIZE] [-o OUT] [--dry-run] mcoolfile\n";
    case program::power_law: return "usage: gd_hic_power_law [--binsize BINSIZE] [--normalize NORMALIZE] [--dry-run] mcool\n";
    case program::compartments: return "usage: gd_hic_compartments [-b BINSIZE] [-n NORM] [-k K] [--exclude X,Y,MT] [--chroms A,B] [--dry-run] coolfile\n";
    default: return "usage: gd_downsample [--rate RATE] [--window WINDOW] [-o OUT] [--dry-run] infile\n";
    }
}

struct options {
    long binsize = 100000;
    bool has_binsize = false;
    long width = 0;                   // -w: the band width of compute_interactions, the width of compute_local_alpha
    std::string normalize = "RAW";
    long rate = 2, window = 0;        // downsample; window 0: the rate
    long components = 3;              // -k
    std::string exclude = "X,Y,MT";   // compartments: chromosomes left out of the mean contact profile
    std::string chroms;               // compartments: the chromosomes to print; empty: all
    std::string output;               // empty: stdout
    bool dry_run = false;
    std::string input;
};

// argparse's conventions: "-o value", "-ovalue", "--opt value" or "--opt=value"; 0 or 2 with a message
inline int parse(program p, int argc, char **argv, options &o, std::string &err)
{
    bool const cooler_short = p == program::interactions || p == program::alpha;
    o.width = p == program::interactions ? 4 : 10;
    using cli::kind;
    static cli::table const cooler_options = {{"--dry-run", kind::flag}, {"-b", kind::value}, {"-w", kind::value}, {"-o", kind::value}},
                            power_law_options = {{"--dry-run", kind::flag}, {"--binsize", kind::value}, {"--normalize", kind::value}},
                            compartments_options = {{"--dry-run", kind::flag}, {"-b", kind::value}, {"-n", kind::value}, {"-k", kind::value}, {"--exclude", kind::value}, {"--chroms", kind::value}},
                            downsample_options = {{"--dry-run", kind::flag}, {"--rate", kind::value}, {"--window", kind::value}, {"-o", kind::value}};
    cli::table const &options = cooler_short ? cooler_options : p == program::power_law ? power_law_options : p == program::compartments ? compartments_options : downsample_options;
    std::vector<std::string> pos;
    err = cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "-o") return o.output = v, std::string();
        if (key == "--normalize" || key == "-n") return o.normalize = v, std::string();
        if (key == "--exclude") return o.exclude = v, std::string();
        if (key == "--chroms") return o.chroms = v, std::string();
        if (key == "-b" || key == "--binsize") return cli::valid_if(o.has_binsize = cli::parse_int(v, o.binsize), v, "int");
        return cli::to_int(v, key == "-w" ? o.width : key == "-k" ? o.components : key == "--rate" ? o.rate : o.window, "int");
    }, pos, cli::shorts::attached);
    if (!err.empty()) return 2;
    char const *what = p == program::power_law ? "mcool" : p == program::downsample ? "infile" : p == program::compartments ? "coolfile" : "mcoolfile";
    if (p == program::interactions && !o.has_binsize) { err = "the following arguments are required: -b"; return 2; }
    if (pos.empty()) { err = std::string("the following arguments are required: ") + what; return 2; }
    if (pos.size() > 1) { err = "unrecognized arguments: " + pos[1]; return 2; }
    o.input = pos[0];
    if (p == program::interactions && (o.width < 2 || o.width > GD_HIC_MAX_BAND)) { err = "argument -w: a band of 2 to " + std::to_string(GD_HIC_MAX_BAND) + " columns"; return 2; }
    if (p == program::alpha && (o.width < 1 || o.width >= GD_HIC_MAX_BAND)) { err = "argument -w: a width of 1 to " + std::to_string(GD_HIC_MAX_BAND - 1); return 2; }
    if (p == program::downsample && (o.rate < 1 || o.window < 0)) { err = "argument --rate: must be at least 1, and --window at least 1"; return 2; }
    if (p == program::compartments && (o.components < 1 || o.components > GD_HIC_MAX_PCS)) { err = "argument -k: 1 to " + std::to_string(GD_HIC_MAX_PCS) + " components"; return 2; }
    if (p != program::downsample && o.binsize < 1) { err = "argument " + std::string(cooler_short || p == program::compartments ? "-b" : "--binsize") + ": must be at least 1"; return 2; }
    return 0;
}

inline std::string signal_header(long W)
{
    std::string h = "chrom\tstart\tend";
    for (long k = 1; k < W; k++) h += "\tD" + std::to_string(k);
    h += "\t";      // the reference joins the two lists with a tab even when the second is empty
    for (long k = 1; k < W - 1; k++) h += (k > 1 ? "\tI" : "I") + std::to_string(k);
    return h;
}

inline void print_plan(program p, options const &o)
{
    std::string const out = o.output.empty() ? "stdout" : o.output;
    if (p == program::downsample) {
        std::printf("rate\t%ld\nwindow\t%ld\nread\t%s\nwrite\t%s\n", o.rate, o.window ? o.window : o.rate, o.input.c_str(), out.c_str());
        return;
    }
    std::string const res = "/resolutions/" + std::to_string(o.binsize);
    std::printf("binsize\t%ld\n", o.binsize);
    if (p == program::compartments) {
        bool const w = o.normalize != "RAW";
        std::string header = "chrom\tstart\tend";
        for (long j = 1; j <= o.components; j++) header += "\tPC" + std::to_string(j);
        std::printf("normalize\t%s\ncomponents\t%ld\nexclude\t%s\nchroms\t%s\n", o.normalize.c_str(), o.components, o.exclude.c_str(), o.chroms.empty() ? "all" : o.chroms.c_str());
        std::printf("read\t%s\t%s/bins/%s\n", o.input.c_str(), res.c_str(), w ? ("{chrom,start,end," + o.normalize + "}").c_str() : "{chrom,start,end}");
        std::printf("read\t%s\t%s/pixels/{bin1_id,bin2_id,count}\n", o.input.c_str(), res.c_str());
        std::printf("write\tstdout\t%s\n", header.c_str());
        return;
    }
    if (p == program::interactions) std::printf("band_width\t%ld\n", o.width);
    if (p == program::alpha) std::printf("width\t%ld\n", o.width);
    if (p == program::power_law) std::printf("normalize\t%s\n", o.normalize.c_str());
    bool const weighted = p == program::power_law && o.normalize != "RAW";
    if (p == program::power_law) std::printf("read\t%s\t%s/bins/%s\n", o.input.c_str(), res.c_str(), weighted ? ("{chrom," + o.normalize + "}").c_str() : "chrom");
    else std::printf("read\t%s\t%s/bins/{chrom,start,end}\n", o.input.c_str(), res.c_str());
    std::printf("read\t%s\t%s/pixels/{bin1_id,bin2_id,count}\n", o.input.c_str(), res.c_str());
    std::printf("write\t%s\t%s\n", out.c_str(),
                p == program::interactions ? signal_header(o.width).c_str() : p == program::alpha ? "chrom\tstart\tend\talpha" : "distance\tcontacts");
}

// Python's format(value, "g"); a NaN of either sign prints "nan"
inline std::string fmt_g(double v)
{
    if (std::isnan(v)) return "nan";
    char buf[64];
    std::snprintf(buf, sizeof buf, "%g", v);
    return buf;
}

struct output {      // the -o file, or stdout
    FILE *f = stdout;
    explicit output(std::string const &path)
    {
        if (path.empty()) return;
        f = std::fopen(path.c_str(), "w");
        if (!f) throw std::runtime_error("cannot write " + path);
    }
    ~output()
    {
        if (f != stdout) std::fclose(f);
        else std::fflush(stdout);
    }
};

// ---- the cooler

struct bin_table {
    std::vector<std::string> names;          // the members of the enum of bins/chrom, in member order
    std::vector<long long> values;           // their codes
    std::vector<int32_t> chrom;              // the code of every bin
    std::vector<long long> start, end;
};

struct pixel_chunk {
    std::vector<int64_t> bin1, bin2;
    std::vector<int32_t> count;
};

constexpr hsize_t kChunkPixels = (hsize_t)1 << 22;      // pixels read and handed over at a time (80 MiB)

struct cooler {
    std::string path, res;
    h5::hid file, group, d1, d2, dc;
    hsize_t n_pixels = 0;

    cooler(std::string const &p, long binsize) : path(p), res("resolutions/" + std::to_string(binsize))
    {
        H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
        file.id = H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
        h5::check(file >= 0, "cannot open " + path);
        h5::check(H5Lexists(file, "resolutions", H5P_DEFAULT) > 0 && H5Lexists(file, res.c_str(), H5P_DEFAULT) > 0, path + ": no /" + res);
        group.id = H5Gopen2(file, res.c_str(), H5P_DEFAULT);
        h5::check(group >= 0, path + ": no /" + res);
        for (char const *need : {"bins", "bins/chrom", "pixels", "pixels/bin1_id", "pixels/bin2_id", "pixels/count"})
            h5::check(H5Lexists(group, need, H5P_DEFAULT) > 0, path + ": no /" + res + "/" + need);
        d1.id = H5Dopen2(group, "pixels/bin1_id", H5P_DEFAULT);
        d2.id = H5Dopen2(group, "pixels/bin2_id", H5P_DEFAULT);
        dc.id = H5Dopen2(group, "pixels/count", H5P_DEFAULT);
        h5::check(d1 >= 0 && d2 >= 0 && dc >= 0, path + ": cannot open the pixel table");
        hsize_t n[3] = {0, 0, 0};
        hid_t const ds[3] = {d1, d2, dc};
        for (int k = 0; k < 3; k++) {
            h5::hid space(H5Dget_space(ds[k]));
            h5::check(H5Sget_simple_extent_ndims(space) == 1, path + ": a pixel column is not one-dimensional");
            H5Sget_simple_extent_dims(space, &n[k], nullptr);
        }
        h5::check(n[0] == n[1] && n[1] == n[2], path + ": the pixel columns differ in length");
        n_pixels = n[0];
    }

    std::vector<long long> read_integers(std::string const &name) const
    {
        std::size_t rows = 0;
        h5::check(H5Lexists(group, name.c_str(), H5P_DEFAULT) > 0, path + ": no /" + res + "/" + name);
        return h5::read_array<long long>(group, name, 1, H5T_NATIVE_LLONG, &rows);
    }

    std::vector<double> read_doubles(std::string const &name) const
    {
        std::size_t rows = 0;
        h5::check(H5Lexists(group, name.c_str(), H5P_DEFAULT) > 0, path + ": no /" + res + "/" + name);
        return h5::read_array<double>(group, name, 1, H5T_NATIVE_DOUBLE, &rows);
    }

    // bins/chrom: the names come from its enum type (h5py.check_dtype(enum=...))
    bin_table read_bins(bool coordinates) const
    {
        bin_table t;
        h5::hid ds(H5Dopen2(group, "bins/chrom", H5P_DEFAULT));
        h5::check(ds >= 0, path + ": cannot open bins/chrom");
        h5::hid type(H5Dget_type(ds)), space(H5Dget_space(ds));
        h5::check(H5Tget_class(type) == H5T_ENUM, path + ": bins/chrom is not an enum of chromosome names");
        h5::hid base(H5Tget_super(type));
        std::size_t const elem = H5Tget_size(type);
        h5::check(elem <= sizeof(long long), path + ": bins/chrom has an integer type wider than 64 bits");
        int const members = H5Tget_nmembers(type);
        for (int m = 0; m < members; m++) {
            char *name = H5Tget_member_name(type, (unsigned)m);
            long long value[2] = {0, 0};
            h5::check(name && H5Tget_member_value(type, (unsigned)m, value) >= 0, path + ": cannot read the enum of bins/chrom");
            h5::check(H5Tconvert(base, H5T_NATIVE_LLONG, 1, value, nullptr, H5P_DEFAULT) >= 0, "cannot convert an enum value");
            t.names.push_back(name);
            t.values.push_back(value[0]);
            H5free_memory(name);
        }
        hssize_t const n = H5Sget_simple_extent_npoints(space);
        h5::check(n > 0 && n < 0x7fffffff, path + ": bins/chrom holds no bin, or 2^31 or more");
        std::vector<long long> raw((std::size_t)n);      // elem <= 8 bytes each, converted in place
        h5::check(H5Dread(ds, type, H5S_ALL, H5S_ALL, H5P_DEFAULT, raw.data()) >= 0, "cannot read bins/chrom");
        h5::check(H5Tconvert(base, H5T_NATIVE_LLONG, (std::size_t)n, raw.data(), nullptr, H5P_DEFAULT) >= 0, "cannot convert bins/chrom");
        t.chrom.resize((std::size_t)n);
        for (std::size_t b = 0; b < (std::size_t)n; b++) {
            h5::check(raw[b] >= INT32_MIN && raw[b] <= INT32_MAX, path + ": a chromosome code does not fit 32 bits");
            t.chrom[b] = (int32_t)raw[b];
        }
        if (coordinates) {
            t.start = read_integers("bins/start");
            t.end = read_integers("bins/end");
            h5::check(t.start.size() == t.chrom.size() && t.end.size() == t.chrom.size(), path + ": bins/start and bins/end differ from bins/chrom in length");
        }
        return t;
    }

    pixel_chunk read_pixels(hsize_t first, hsize_t n) const
    {
        pixel_chunk c;
        c.bin1.resize(n);
        c.bin2.resize(n);
        c.count.resize(n);
        h5::hid mem(H5Screate_simple(1, &n, nullptr));
        auto read = [&](hid_t ds, hid_t type, void *out) {
            h5::hid space(H5Dget_space(ds));
            H5Sselect_hyperslab(space, H5S_SELECT_SET, &first, nullptr, &n, nullptr);
            h5::check(H5Dread(ds, type, mem, space, H5P_DEFAULT, out) >= 0, path + ": cannot read the pixel table");
        };
        read(d1, H5T_NATIVE_INT64, c.bin1.data());
        read(d2, H5T_NATIVE_INT64, c.bin2.data());
        read(dc, H5T_NATIVE_INT32, c.count.data());
        return c;
    }
};

using device = cli::handle<gd_hic, gd_hic_destroy>;

inline void open(device &dev, bin_table const &bins)
{
    dev.open([&bins](gd_hic **h) { gd_hic_desc const d{0, 0}; return gd_hic_create(&d, bins.chrom.data(), (uint32_t)bins.chrom.size(), h); });
}

// one pass: chunk k + 1 is read on a second thread while the device accumulates chunk k
inline void stream_pixels(cooler const &c, device &dev, cli::stopwatch &sw)
{
    auto fetch = [&c](hsize_t first) { return c.read_pixels(first, std::min<hsize_t>(kChunkPixels, c.n_pixels - first)); };
    std::future<pixel_chunk> next;
    if (c.n_pixels) next = std::async(std::launch::async, fetch, (hsize_t)0);
    for (hsize_t first = 0; first < c.n_pixels; first += kChunkPixels) {
        pixel_chunk const chunk = next.get();
        if (first + kChunkPixels < c.n_pixels) next = std::async(std::launch::async, fetch, first + kChunkPixels);
        sw.read += sw.lap();
        cli::check(gd_hic_accumulate(dev.h, chunk.bin1.data(), chunk.bin2.data(), chunk.count.data(), chunk.count.size()));
        sw.compute += sw.lap();
    }
}

// the (first, end) run of every enum member's code; the bins of one chromosome must be contiguous
inline std::map<long long, std::pair<std::size_t, std::size_t>> runs_by_code(bin_table const &bins, std::string const &path)
{
    std::map<long long, std::pair<std::size_t, std::size_t>> runs;
    for (std::size_t b = 0; b < bins.chrom.size();) {
        std::size_t e = b + 1;
        while (e < bins.chrom.size() && bins.chrom[e] == bins.chrom[b]) e++;
        h5::check(runs.emplace(bins.chrom[b], std::make_pair(b, e)).second, path + ": the bins of chromosome code " + std::to_string(bins.chrom[b]) + " are not contiguous");
        b = e;
    }
    return runs;
}

inline std::string strip_chr(std::string const &name) { return name.compare(0, 3, "chr") == 0 ? name.substr(3) : name; }

// by_std_chrom_order: (0, number) for numbered chromosomes, then X, Y, MT / M; false for any other name (the reference's KeyError)
inline bool std_chrom_order(std::string const &name, std::pair<long, long> &key)
{
    std::string const s = strip_chr(name);
    long n = 0;
    if (cli::parse_int(s, n)) { key = {0, n}; return true; }
    static std::map<std::string, long> const rank = {{"X", 1}, {"Y", 2}, {"MT", 3}, {"M", 3}};
    auto const it = rank.find(s);
    if (it == rank.end()) return false;
    key = {it->second, 0};
    return true;
}

// ---- compute_interactions

inline void run_interactions(options const &o)
{
    cli::stopwatch sw;
    cooler c(o.input, o.binsize);
    bin_table const bins = c.read_bins(true);
    auto const runs = runs_by_code(bins, o.input);
    struct entry { std::pair<long, long> key; std::string name; long long code; };
    std::vector<entry> order;
    for (std::size_t m = 0; m < bins.names.size(); m++) {
        if (bins.names[m] == "MT") continue;      // BLACKLISTED_CHROMS
        entry e{{0, 0}, bins.names[m], bins.values[m]};
        if (!std_chrom_order(e.name, e.key)) throw std::runtime_error(o.input + ": chromosome name '" + e.name + "' has no standard order");
        order.push_back(e);
    }
    std::stable_sort(order.begin(), order.end(), [](entry const &a, entry const &b) { return a.key < b.key; });
    output out(o.output);
    sw.read += sw.lap();
    device dev;
    open(dev, bins);
    int32_t band = -1;
    uint32_t const W = (uint32_t)o.width;
    cli::check(gd_hic_add_band(dev.h, W, &band));
    sw.compute += sw.lap();
    stream_pixels(c, dev, sw);
    std::size_t const n = bins.chrom.size();
    std::vector<double> D(n * (W - 1)), I(n * (W - 2));
    cli::check(gd_hic_decay_insulation(dev.h, band, D.data(), I.data()));
    sw.compute += sw.lap();
    std::fprintf(out.f, "%s\n", signal_header(o.width).c_str());
    std::string line;
    for (auto const &e : order) {
        auto const it = runs.find(e.code);
        if (it == runs.end()) continue;      // a name without bins: an empty track
        std::string const name = e.name.compare(0, 3, "chr") == 0 ? e.name : "chr" + e.name;
        for (std::size_t b = it->second.first; b < it->second.second; b++) {
            line = name + "\t" + std::to_string(bins.start[b]) + "\t" + std::to_string(bins.end[b]) + "\t";
            for (uint32_t k = 0; k + 1 < W; k++) line += (k ? "\t" : "") + fmt_g(D[b * (W - 1) + k]);
            line += "\t";
            for (uint32_t k = 0; k + 2 < W; k++) line += (k ? "\t" : "") + fmt_g(I[b * (W - 2) + k]);
            std::fprintf(out.f, "%s\n", line.c_str());
        }
    }
    sw.write += sw.lap();
    sw.report("gd_compute_interactions");
    dev.report("gd_compute_interactions");
}

// ---- compute_local_alpha

inline void run_alpha(options const &o)
{
    cli::stopwatch sw;
    cooler c(o.input, o.binsize);
    bin_table const bins = c.read_bins(true);
    // enumerate_runs; the reference looks the run of a chromosome up by its code: chrom_ranges[key]
    std::vector<std::pair<std::size_t, std::size_t>> runs;
    for (std::size_t b = 0; b < bins.chrom.size();) {
        std::size_t e = b + 1;
        while (e < bins.chrom.size() && bins.chrom[e] == bins.chrom[b]) e++;
        runs.emplace_back(b, e);
        b = e;
    }
    for (std::size_t m = 0; m < bins.names.size(); m++)
        if (bins.values[m] < 0 || (std::size_t)bins.values[m] >= runs.size())
            throw std::runtime_error(o.input + ": chromosome '" + bins.names[m] + "' has code " + std::to_string(bins.values[m]) + ", but the bin table has " +
                                     std::to_string(runs.size()) + " runs of equal codes");      // IndexError
    output out(o.output);
    sw.read += sw.lap();
    device dev;
    open(dev, bins);
    int32_t band = -1;
    cli::check(gd_hic_add_band(dev.h, (uint32_t)o.width + 1, &band));
    sw.compute += sw.lap();
    stream_pixels(c, dev, sw);
    std::vector<double> alpha(bins.chrom.size());
    cli::check(gd_hic_local_alpha(dev.h, band, alpha.data()));
    sw.compute += sw.lap();
    std::fputs("chrom\tstart\tend\talpha\n", out.f);
    for (std::size_t m = 0; m < bins.names.size(); m++) {
        auto const &r = runs[(std::size_t)bins.values[m]];
        for (std::size_t b = r.first; b < r.second; b++)
            std::fprintf(out.f, "%s\t%lld\t%lld\t%s\n", bins.names[m].c_str(), bins.start[b], bins.end[b], fmt_g(alpha[b]).c_str());
    }
    sw.write += sw.lap();
    sw.report("gd_compute_local_alpha");
    dev.report("gd_compute_local_alpha");
}

// ---- hic_power_law

inline void run_power_law(options const &o)
{
    cli::stopwatch sw;
    cooler c(o.input, o.binsize);
    bin_table const bins = c.read_bins(false);
    std::size_t const n = bins.chrom.size();
    bool const weighted = o.normalize != "RAW";
    std::vector<double> weights;
    if (weighted) {
        weights = c.read_doubles("bins/" + o.normalize);
        h5::check(weights.size() == n, o.input + ": bins/" + o.normalize + " differs from bins/chrom in length");
    }
    std::vector<uint8_t> excluded(n, 0);
    std::map<long long, uint32_t> sizes;
    for (std::size_t m = 0; m < bins.names.size(); m++) {
        std::string const s = strip_chr(bins.names[m]);
        if (s != "X" && s != "Y" && s != "MT") continue;      // BLACKLISTED_CHROMS
        for (std::size_t b = 0; b < n; b++)
            if (bins.chrom[b] == bins.values[m]) excluded[b] = 1;
    }
    uint32_t size = 0;
    for (std::size_t b = 0; b < n; b++) size = std::max(size, ++sizes[bins.chrom[b]]);
    sw.read += sw.lap();
    device dev;
    open(dev, bins);
    int32_t profile = -1;
    cli::check(gd_hic_add_distance_profile(dev.h, excluded.data(), weighted ? weights.data() : nullptr, size, &profile));
    sw.compute += sw.lap();
    stream_pixels(c, dev, sw);
    std::vector<double> mean(size);
    cli::check(gd_hic_fetch_profile(dev.h, profile, nullptr, nullptr, mean.data()));
    sw.compute += sw.lap();
    std::puts("distance\tcontacts");
    for (uint32_t d = 0; d < size; d++) std::printf("%lld\t%s\n", (long long)d * o.binsize, fmt_g(mean[d]).c_str());
    std::fflush(stdout);
    sw.write += sw.lap();
    sw.report("gd_hic_power_law");
    dev.report("gd_hic_power_law");
}

// ---- compartments: dense cis matrices, observed / expected, the leading principal components of every requested chromosome

inline std::vector<std::string> split_commas(std::string const &s)
{
    std::vector<std::string> out;
    for (std::size_t at = 0; at <= s.size();) {
        auto const next = std::min(s.find(',', at), s.size());
        if (next > at) out.push_back(s.substr(at, next - at));
        at = next + 1;
    }
    return out;
}

inline void run_compartments(options const &o)
{
    cli::stopwatch sw;
    cooler c(o.input, o.binsize);
    bin_table const bins = c.read_bins(true);
    std::size_t const n = bins.chrom.size();
    auto const runs = runs_by_code(bins, o.input);
    bool const weighted = o.normalize != "RAW";
    std::vector<double> weights;
    if (weighted) {
        weights = c.read_doubles("bins/" + o.normalize);
        h5::check(weights.size() == n, o.input + ": bins/" + o.normalize + " differs from bins/chrom in length");
    }
    auto listed = [](std::vector<std::string> const &list, std::string const &name) {
        for (auto const &l : list)
            if (strip_chr(l) == strip_chr(name)) return true;
        return false;
    };
    auto const exclude = split_commas(o.exclude), wanted = split_commas(o.chroms);
    for (auto const &w : wanted)
        if (!listed(bins.names, w)) throw std::runtime_error(o.input + ": no chromosome '" + w + "'");
    std::vector<uint8_t> excluded(n, 0);
    for (std::size_t m = 0; m < bins.names.size(); m++) {
        auto const it = runs.find(bins.values[m]);
        if (it == runs.end() || !listed(exclude, bins.names[m])) continue;
        std::fill(excluded.begin() + (long)it->second.first, excluded.begin() + (long)it->second.second, 1);
    }
    sw.read += sw.lap();
    device dev;
    open(dev, bins);
    int32_t dense = -1;
    cli::check(gd_hic_add_dense(dev.h, weighted ? weights.data() : nullptr, &dense));
    sw.compute += sw.lap();
    stream_pixels(c, dev, sw);
    cli::check(gd_hic_dense_profile(dev.h, dense, excluded.data(), nullptr, nullptr, nullptr));
    std::vector<uint8_t> valid(n);
    cli::check(gd_hic_dense_valid(dev.h, dense, valid.data()));
    uint32_t const k = (uint32_t)o.components;
    struct result { std::size_t member; std::vector<double> pcs; };
    std::vector<result> results;
    for (std::size_t m = 0; m < bins.names.size(); m++) {
        auto const it = runs.find(bins.values[m]);
        if (it == runs.end() || (!wanted.empty() && !listed(wanted, bins.names[m]))) continue;
        std::size_t const beg = it->second.first, size = it->second.second - beg;
        result r{m, std::vector<double>(size * k)};
        std::vector<double> variances(k);
        int32_t iterations = 0;
        if (gd_hic_dense_pca(dev.h, dense, (int32_t)bins.values[m], GD_HIC_DENSE_ENRICHMENT, valid.data() + beg, k, r.pcs.data(), variances.data(), nullptr, &iterations))
            throw std::runtime_error("chromosome " + bins.names[m] + ": " + gd_last_error());
        std::string line = "# " + bins.names[m] + " variances";
        for (double v : variances) line += " " + fmt_g(v);
        std::printf("%s iterations %d\n", line.c_str(), iterations);
        results.push_back(std::move(r));
    }
    sw.compute += sw.lap();
    std::string header = "chrom\tstart\tend";
    for (uint32_t j = 1; j <= k; j++) header += "\tPC" + std::to_string(j);
    std::puts(header.c_str());
    for (auto const &r : results) {
        auto const &run = runs.find(bins.values[r.member])->second;
        for (std::size_t b = run.first; b < run.second; b++) {
            std::string line = bins.names[r.member] + "\t" + std::to_string(bins.start[b]) + "\t" + std::to_string(bins.end[b]);
            for (uint32_t j = 0; j < k; j++) line += "\t" + fmt_g(r.pcs[(b - run.first) * k + j]);
            std::puts(line.c_str());
        }
    }
    std::fflush(stdout);
    sw.write += sw.lap();
    sw.report("gd_hic_compartments");
    dev.report("gd_hic_compartments");
}

// ---- downsample: host only

inline std::vector<std::string> split_tabs(std::string const &s)
{
    std::vector<std::string> out;
    std::size_t at = 0;
    for (;;) {
        auto const next = s.find('\t', at);
        out.push_back(s.substr(at, next == std::string::npos ? next : next - at));
        if (next == std::string::npos) return out;
        at = next + 1;
    }
}

// pandas.read_csv: an empty field and the usual spellings of a missing value are NaN
inline double parse_value(std::string const &s, std::string const &where)
{
    static char const *const missing[] = {"", "NA", "N/A", "NaN", "nan", "NULL", "null", "None", "#N/A", "n/a", "<NA>", "-NaN", "-nan"};
    for (auto m : missing)
        if (s == m) return std::nan("");
    double v = 0;
    if (!cli::parse_float(s, v)) throw std::runtime_error(where + ": '" + s + "' is not a number");
    return v;
}

inline void run_downsample(options const &o)
{
    std::ifstream in(o.input);
    if (!in) throw std::runtime_error("cannot read " + o.input);
    std::string header, line;
    if (!std::getline(in, header)) throw std::runtime_error(o.input + ": no header line");
    std::size_t const columns = split_tabs(header).size();
    if (columns < 3) throw std::runtime_error(o.input + ": fewer than the three columns chrom, start, end");
    struct track { std::string chrom; std::vector<std::string> start, end; std::vector<double> values; };
    std::vector<track> tracks;                          // groupby(sort=False): in the order of first appearance
    std::map<std::string, std::size_t> index;
    for (std::size_t row = 2; std::getline(in, line); row++) {
        if (line.empty()) continue;
        auto const f = split_tabs(line);
        std::string const where = o.input + ":" + std::to_string(row);
        if (f.size() != columns) throw std::runtime_error(where + ": " + std::to_string(f.size()) + " fields, the header has " + std::to_string(columns));
        auto it = index.find(f[0]);
        if (it == index.end()) {
            it = index.emplace(f[0], tracks.size()).first;
            tracks.push_back(track{f[0], {}, {}, {}});
        }
        track &t = tracks[it->second];
        t.start.push_back(f[1]);
        t.end.push_back(f[2]);
        for (std::size_t k = 3; k < columns; k++) t.values.push_back(parse_value(f[k], where));
    }
    output out(o.output);
    std::fprintf(out.f, "%s\n", header.c_str());
    long const rate = o.rate, window = o.window ? o.window : o.rate;
    std::size_t const cols = columns - 3;
    for (auto const &t : tracks) {
        long const n = (long)t.start.size();
        for (long m = 0; m * rate < n; m++) {
            std::string row = t.chrom + "\t" + t.start[(std::size_t)(rate * m)] + "\t" + t.end[(std::size_t)(std::min(rate * m + rate, n) - 1)] + "\t";
            long const lo = std::max(rate * (m + 1) - window + 1, 0L), hi = std::min(rate * (m + 1), n - 1);
            for (std::size_t k = 0; k < cols; k++) {
                double sum = 0;
                long count = 0;
                for (long r = lo; r <= hi; r++) {
                    double const v = t.values[(std::size_t)r * cols + k];
                    if (std::isnan(v)) continue;
                    sum += v;
                    count++;
                }
                row += (k ? "\t" : "") + fmt_g(count ? sum / (double)count : std::nan(""));
            }
            std::fprintf(out.f, "%s\n", row.c_str());
        }
    }
}

// status 0, 1 (error: <what>) or 2 (usage)
inline int main(program p, int argc, char **argv)
{
    options o;
    return cli::run(usage(p), name_of(p), "error:", [&](std::string &err) { return parse(p, argc, argv, o, err); },
                    [&] { return o.dry_run && (print_plan(p, o), true); }, [&] {
        if (p == program::interactions) run_interactions(o);
        else if (p == program::alpha) run_alpha(o);
        else if (p == program::power_law) run_power_law(o);
        else if (p == program::compartments) run_compartments(o);
        else run_downsample(o);
        return 0;
    });
}

}  // namespace hic
}  // namespace gd
