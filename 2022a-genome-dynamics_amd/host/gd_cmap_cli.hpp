// gd_cmap_cli.hpp -- what gd_contact_map, gd_nad_profile, gd_gw_contact_matrix and gd_power_law share: the command lines of
// the reference's 5-sim-genome/src/{contact_map, nad_profile, gw_contact_matrix, power_law} (__main__.py), their reads of a
// trajectory file (the metadata, the frames they select and the stored contact maps) and their outputs.  The sums are
// libgdyn's (include/gdyn_cmap.h); the HDF5 helpers are the programs' shared ones (gd_cli_util.hpp).
//
// Deviations from the reference, all documented in DESIGN.md section 7d: --chroms and --output are required (the reference's
// defaults die in None.split and h5py.File(None)); a --frame-range of more than two tokens is a usage error; the NAD profile
// is the true sum (the reference's fancy-index += depends on the HDF5 chunk layout); a row whose index lies beyond
// particle_types is not nucleolar (the reference raises IndexError).
#pragma once
#include <glob.h>

#include <future>
#include <map>
#include <memory>

#include <json.hpp>   // nlohmann/json single header

#include "../../include/gdyn_cmap.h"
#include "gd_cli_util.hpp"

namespace gd {
namespace cmap {

enum class program { contact_map, nad_profile, gw_contact_matrix, power_law };

inline const char *name_of(program p)
{
    switch (p) {
    case program::contact_map: return "gd_contact_map";
    case program::nad_profile: return "gd_nad_profile";
    case program::gw_contact_matrix: return "gd_gw_contact_matrix";
    default: return "gd_power_law";
    }
}

inline const char *usage(program p)
{
    switch (p) {
    case program::contact_map: return "usage: gd_contact_map [--after AFTER] [--before BEFORE] --chroms CHROMS [--dry-run] jobdir\n";
    case program::nad_profile: return "usage: gd_nad_profile [--after AFTER] [--before BEFORE] --chroms CHROMS [--dry-run] jobdir\n";
    case program::gw_contact_matrix:
        return "usage: gd_gw_contact_matrix [--frame-range START[:END]] [--rebin-rate RATE] --output OUTPUT [--dry-run] inputs ...\n";
    default: return "usage: gd_power_law [--dry-run] trajfiles ...\n";
    }
}

struct options {
    bool has_before = false, has_after = false;
    long before = 0, after = 0;
    std::vector<std::string> chroms;
    int range_tokens = 0;             // --frame-range: 0 = every frame, 1 = (a, None), 2 = (a, b)
    long range_a = 0, range_b = 0;
    long rebin_rate = 1;
    std::string output;
    bool dry_run = false;
    std::vector<std::string> inputs;  // jobdir, inputs or trajfiles
};

inline std::vector<std::string> split(std::string const &s, char sep)      // str.split(sep)
{
    std::vector<std::string> out;
    std::size_t at = 0;
    for (;;) {
        auto const next = s.find(sep, at);
        out.push_back(s.substr(at, next == std::string::npos ? next : next - at));
        if (next == std::string::npos) return out;
        at = next + 1;
    }
}

// argparse's conventions: "--opt value" or "--opt=value"; 0 or 2 with a message
inline int parse(program p, int argc, char **argv, options &o, std::string &err)
{
    bool const by_step = p == program::contact_map || p == program::nad_profile, gw = p == program::gw_contact_matrix;
    using cli::kind;
    static cli::table const by_step_options = {{"--dry-run", kind::flag}, {"--after", kind::value}, {"--before", kind::value}, {"--chroms", kind::value}},
                            gw_options = {{"--dry-run", kind::flag}, {"--frame-range", kind::value}, {"--rebin-rate", kind::value}, {"--output", kind::value}, {"-o", kind::value}},
                            power_law_options = {{"--dry-run", kind::flag}};
    bool has_chroms = false;
    err = cli::scan(argc, argv, by_step ? by_step_options : gw ? gw_options : power_law_options, [&](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--after") return cli::valid_if(o.has_after = cli::parse_int(v, o.after), v, "int");
        if (key == "--before") return cli::valid_if(o.has_before = cli::parse_int(v, o.before), v, "int");
        if (key == "--rebin-rate") return cli::to_int(v, o.rebin_rate, "int");
        if (key == "--chroms") return has_chroms = true, o.chroms = split(v, ','), std::string();
        if (key != "--frame-range") return o.output = v, std::string();
        auto const tokens = split(v, ':');
        // the reference leaves three tokens or more as a string, which fails in slice(*frame_range)
        if (tokens.size() > 2) return "expected START[:END], got '" + v + "'";
        o.range_tokens = (int)tokens.size();
        bool const ok = cli::parse_int(tokens[0], o.range_a) && (tokens.size() < 2 || cli::parse_int(tokens[1], o.range_b));
        return ok ? std::string() : "invalid int value in '" + v + "'";
    }, o.inputs);
    if (!err.empty()) return 2;
    if (by_step) {
        if (!has_chroms) { err = "the following arguments are required: --chroms"; return 2; }
        if (o.inputs.empty()) { err = "the following arguments are required: jobdir"; return 2; }
        if (o.inputs.size() > 1) { err = "unrecognized arguments: " + o.inputs[1]; return 2; }
    } else if (gw) {
        if (o.output.empty()) { err = "the following arguments are required: --output/-o"; return 2; }
        if (o.inputs.empty()) { err = "the following arguments are required: inputs"; return 2; }
        if (o.rebin_rate < 1) { err = "argument --rebin-rate: must be at least 1"; return 2; }
    } else if (o.inputs.empty()) {
        err = "the following arguments are required: trajfiles";
        return 2;
    }
    return 0;
}

inline void print_plan(program p, options const &o)
{
    auto opt = [](bool has, long v) { return has ? std::to_string(v) : std::string("None"); };
    if (p == program::contact_map || p == program::nad_profile) {
        std::printf("before\t%s\nafter\t%s\n", opt(o.has_before, o.before).c_str(), opt(o.has_after, o.after).c_str());
        for (auto const &c : o.chroms) std::printf("chrom\t%s\n", c.c_str());
        std::printf("read\t%s/output-*.h5\t/metadata/%s\n", o.inputs[0].c_str(),
                    p == program::nad_profile ? "{chromosome_ranges,particle_types}" : "chromosome_ranges");
        std::printf("read\t%s/output-*.h5\t/snapshots/interphase/<step>/contact_map\n", o.inputs[0].c_str());
        std::printf("write\tstdout\t%s\n", p == program::nad_profile ? "profile" : "matrix");
    } else if (p == program::gw_contact_matrix) {
        std::printf("frame_range\t%s\t%s\n", opt(o.range_tokens >= 1, o.range_a).c_str(), opt(o.range_tokens == 2, o.range_b).c_str());
        std::printf("rebin_rate\t%ld\n", o.rebin_rate);
        std::printf("read\t%s\t/metadata/chromosome_ranges\n", o.inputs[0].c_str());
        for (auto const &t : o.inputs) std::printf("read\t%s\t/snapshots/interphase/<step>/contact_map\n", t.c_str());
        std::printf("write\t%s\t/metadata/{chromosome_ranges,rebin_map}\n", o.output.c_str());
        std::printf("write\t%s\t/contact_matrix\n", o.output.c_str());
    } else {
        for (auto const &t : o.inputs) {
            std::printf("read\t%s\t/metadata/{particle_types,chromosome_ranges}\n", t.c_str());
            std::printf("read\t%s\t/snapshots/interphase/<last step with a map>/contact_map\n", t.c_str());
        }
        std::printf("write\tstdout\texponents\n");
    }
}

using device = cli::handle<gd_cmap, gd_cmap_destroy>;      // opened when the first file has been read: a missing input is reported as such

inline void open(device &dev, int ordinal = 0)      // ordinal: the HIP device
{
    dev.open([ordinal](gd_cmap **h) { gd_cmap_desc const d{ordinal, 0}; return gd_cmap_create(&d, h); });
}

inline std::vector<int32_t> fetch(device &dev, int32_t target)
{
    uint64_t count = 0;
    cli::check(gd_cmap_target_size(dev.h, target, &count));
    std::vector<int32_t> out(count);
    cli::check(gd_cmap_fetch(dev.h, target, out.data()));
    return out;
}

// ---- what is read from one trajectory file

enum class frames { none, by_step, by_slice, last_with_map };

struct request {
    frames how = frames::by_step;
    options const *o = nullptr;
    bool types = false;        // particle_types and the value of "nucleolus"
};

struct trajectory {
    std::vector<int> ranges;                     // (K, 2) chromosome_ranges
    std::map<std::string, std::size_t> keys;     // chromosome name -> row
    std::vector<std::string> names;              // row -> name
    std::size_t n_particles = 0;                 // length of particle_types (when asked for)
    std::vector<uint8_t> is_nucleolus;
    bool nucleolus_member = false;               // the enum of particle_types has "nucleolus"
    std::vector<uint32_t> rows;                  // the contact maps of the selected frames, one after the other
    std::size_t maps = 0;
};

inline void read_ranges(hid_t file, std::string const &path, trajectory &t)
{
    h5::hid meta(H5Gopen2(file, "/metadata", H5P_DEFAULT));
    h5::check(meta >= 0, path + ": no /metadata");
    std::size_t rows = 0;
    t.ranges = h5::read_array<int>(meta, "chromosome_ranges", 2, H5T_NATIVE_INT, &rows);
    h5::hid rds(H5Dopen2(meta, "chromosome_ranges", H5P_DEFAULT)), attr(H5Aopen(rds, "keys", H5P_DEFAULT));
    h5::check(attr >= 0, path + ": chromosome_ranges has no 'keys' attribute");
    auto const keys = nlohmann::json::parse(h5::read_string_from(attr, true));
    t.names.assign(rows, "");
    for (auto it = keys.begin(); it != keys.end(); ++it) {
        std::size_t const row = it.value().get<std::size_t>();
        t.keys[it.key()] = row;
        if (row < rows) t.names[row] = it.key();
    }
    for (std::size_t k = 0; k < rows; k++)
        h5::check(t.ranges[2 * k] >= 0 && t.ranges[2 * k + 1] >= t.ranges[2 * k], path + ": chromosome_ranges holds a reversed or negative range");
}

// the chromosome table alone: of a prepared input as well, which has no /snapshots/interphase yet
inline trajectory load_ranges(std::string const &path)
{
    trajectory t;
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    hid_t const file = H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
    h5::check(file >= 0, "cannot open " + path);
    // closed here (h5::hid does not close files): gd_interphase opens the same file for writing next
    try {
        read_ranges(file, path, t);
    } catch (...) {
        H5Fclose(file);
        throw;
    }
    H5Fclose(file);
    return t;
}

// nad_profile.py:46-57: the phase's own metadata group if it has particle_types, else the file's
inline void read_types(hid_t file, std::string const &path, trajectory &t)
{
    std::string where = "/metadata";
    if (H5Lexists(file, "/snapshots/interphase/metadata", H5P_DEFAULT) > 0 && H5Lexists(file, "/snapshots/interphase/metadata/particle_types", H5P_DEFAULT) > 0)
        where = "/snapshots/interphase/metadata";
    h5::hid ds(H5Dopen2(file, (where + "/particle_types").c_str(), H5P_DEFAULT));
    h5::check(ds >= 0, path + ": missing dataset " + where + "/particle_types");
    h5::hid type(H5Dget_type(ds)), space(H5Dget_space(ds));
    hssize_t const n = H5Sget_simple_extent_npoints(space);
    std::size_t const elem = H5Tget_size(type);
    t.n_particles = (std::size_t)std::max<hssize_t>(n, 0);
    std::vector<unsigned char> raw(t.n_particles * elem);
    if (n > 0) h5::check(H5Dread(ds, type, H5S_ALL, H5S_ALL, H5P_DEFAULT, raw.data()) >= 0, "cannot read particle_types");
    t.is_nucleolus.assign(t.n_particles, 0);
    if (H5Tget_class(type) != H5T_ENUM) return;      // no enum: power_law only needs the length
    std::vector<unsigned char> value(elem);
    if (H5Tenum_valueof(type, "nucleolus", value.data()) < 0) return;      // the caller that needs it says so
    for (std::size_t k = 0; k < t.n_particles; k++) t.is_nucleolus[k] = std::memcmp(raw.data() + k * elem, value.data(), elem) == 0;
    t.nucleolus_member = true;
}

// Python's slice(a, b).indices(n) for step 1
inline std::pair<std::size_t, std::size_t> slice_bounds(options const &o, std::size_t n)
{
    auto clamp = [n](long v) { return (std::size_t)std::min<long>(std::max<long>(v < 0 ? v + (long)n : v, 0), (long)n); };
    std::size_t const lo = o.range_tokens >= 1 ? clamp(o.range_a) : 0, hi = o.range_tokens == 2 ? clamp(o.range_b) : n;
    return {lo, std::max(lo, hi)};
}

inline trajectory load(std::string const &path, request const &rq)
{
    trajectory t;
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);      // the error stack of a thread-safe library is the calling thread's
    h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    h5::check(file >= 0, "cannot open " + path);
    read_ranges(file, path, t);
    if (rq.types) read_types(file, path, t);
    h5::hid phase(H5Gopen2(file, "/snapshots/interphase", H5P_DEFAULT));
    h5::check(phase >= 0, path + ": no /snapshots/interphase");
    auto const steps = h5::read_string_list(phase, ".steps");
    std::vector<std::string> chosen;
    if (rq.how == frames::by_step) {
        for (auto const &s : steps) {
            long v = 0;
            h5::check(cli::parse_int(s, v), path + ": step '" + s + "' is not an integer");
            if ((!rq.o->has_before || v < rq.o->before) && (!rq.o->has_after || v >= rq.o->after)) chosen.push_back(std::to_string(v));
        }
    } else if (rq.how == frames::by_slice) {
        auto const b = slice_bounds(*rq.o, steps.size());
        chosen.assign(steps.begin() + (long)b.first, steps.begin() + (long)b.second);
    } else if (rq.how == frames::last_with_map) {
        chosen.assign(steps.rbegin(), steps.rend());
    }
    for (auto const &s : chosen) {
        h5::hid snap(H5Gopen2(phase, s.c_str(), H5P_DEFAULT));
        h5::check(snap >= 0, path + ": missing snapshot " + s);
        if (!h5::exists(snap, "contact_map")) continue;      // the map is not saved in every frame
        auto const rows = h5::read_array<uint32_t>(snap, "contact_map", 3, H5T_NATIVE_UINT32);
        t.rows.insert(t.rows.end(), rows.begin(), rows.end());
        t.maps++;
        if (rq.how == frames::last_with_map) break;
    }
    return t;
}

// loads file k + 1 on a second thread while the caller works on file k
struct prefetcher {
    std::vector<std::string> const &paths;
    request rq;
    std::future<trajectory> next;
    std::size_t at = 0;
    prefetcher(std::vector<std::string> const &p, request r) : paths(p), rq(r) { start(); }
    void start()
    {
        if (at < paths.size()) next = std::async(std::launch::async, load, paths[at], rq);
    }
    trajectory take()
    {
        trajectory t = next.get();
        at++;
        start();
        return t;
    }
};

// ---- contact_map and nad_profile

inline std::vector<std::string> job_files(std::string const &jobdir)
{
    glob_t g{};
    std::vector<std::string> out;
    if (glob((jobdir + "/output-*.h5").c_str(), 0, nullptr, &g) == 0)
        for (std::size_t k = 0; k < g.gl_pathc; k++) out.push_back(g.gl_pathv[k]);
    globfree(&g);
    if (out.empty()) throw std::runtime_error("no output-*.h5 in " + jobdir);      // np.savetxt(None) in the reference
    return out;
}

inline void run_by_step(program p, options const &o)
{
    bool const nad = p == program::nad_profile;
    auto const files = job_files(o.inputs[0]);
    cli::stopwatch sw;
    request rq;
    rq.o = &o;
    rq.types = nad;
    prefetcher pf(files, rq);
    device dev;
    std::vector<long long> sum;
    std::size_t side = 0;
    bool first = true;
    for (std::size_t k = 0; k < files.size(); k++) {
        trajectory t = pf.take();
        sw.read += sw.lap();
        if (nad && !t.nucleolus_member) throw std::runtime_error(files[k] + ": particle_types has no enum member 'nucleolus'");      // KeyError
        open(dev);
        cli::check(gd_cmap_clear(dev.h));
        std::vector<int32_t> targets;
        for (auto const &c : o.chroms) {
            auto const it = t.keys.find(c);
            if (it == t.keys.end() || it->second * 2 + 1 >= t.ranges.size()) throw std::runtime_error(files[k] + ": no chromosome '" + c + "'");      // KeyError
            uint32_t const beg = (uint32_t)t.ranges[2 * it->second], end = (uint32_t)t.ranges[2 * it->second + 1];
            int32_t id = -1;
            if (nad) cli::check(gd_cmap_add_nucleolus_profile(dev.h, beg, end, t.is_nucleolus.data(), (uint32_t)t.n_particles, &id));
            else cli::check(gd_cmap_add_region(dev.h, beg, end, &id));
            targets.push_back(id);
        }
        cli::check(gd_cmap_accumulate(dev.h, t.rows.data(), t.rows.size() / 3));
        for (auto id : targets) {
            if (!nad) cli::check(gd_cmap_finish(dev.h, id));
            auto const part = fetch(dev, id);
            if (first) {
                sum.assign(part.begin(), part.end());
                side = part.size();
                first = false;
                continue;
            }
            // numpy's += of arrays of different shapes
            if (part.size() != side) throw std::runtime_error("chromosomes of different sizes cannot be summed (" + std::to_string(side) + " and " + std::to_string(part.size()) + " values)");
            for (std::size_t e = 0; e < side; e++) sum[e] += part[e];
        }
        sw.compute += sw.lap();
    }
    std::size_t n = side;
    if (!nad) {
        n = 0;
        while (n * n < side) n++;
    }
    std::string line;
    if (nad) {
        for (std::size_t e = 0; e < side; e++) std::printf("%lld\n", sum[e]);
    } else {
        for (std::size_t r = 0; r < n; r++) {
            line.clear();
            for (std::size_t c = 0; c < n; c++) {
                if (c) line += '\t';
                line += std::to_string(sum[r * n + c]);
            }
            std::puts(line.c_str());
        }
    }
    sw.write += sw.lap();
    sw.report(name_of(p));
    dev.report(name_of(p));
}

// ---- gw_contact_matrix

struct rebinning {
    std::vector<int32_t> map, binned;      // rebin_map; (K, 2) binned ranges
    uint32_t n_bins = 0;
};

// determine_rebin_map (command.py:103-126)
inline rebinning rebin(trajectory const &t, long rate)
{
    rebinning r;
    int n_src = 0;
    for (int v : t.ranges) n_src = std::max(n_src, v);
    r.map.assign((std::size_t)n_src, 0);
    int32_t chrom_start = 0;
    for (std::size_t k = 0; k + 1 < t.ranges.size(); k += 2) {
        int const start = t.ranges[k], end = t.ranges[k + 1];
        if (end == start) throw std::runtime_error("chromosome_ranges holds an empty range");      // bins[-1] of an empty array
        for (int b = start; b < end; b++) r.map[(std::size_t)b] = (int32_t)((b - start) / rate) + chrom_start;
        int32_t const chrom_end = chrom_start + (int32_t)((end - start - 1) / rate) + 1;
        r.binned.push_back(chrom_start);
        r.binned.push_back(chrom_end);
        chrom_start = chrom_end;
    }
    for (auto v : r.binned) r.n_bins = std::max<uint32_t>(r.n_bins, (uint32_t)v);
    return r;
}

// save_contact_matrix (command.py): h5py.File(filename, "w") with /contact_matrix, /metadata/chromosome_ranges (the binned
// ranges, typed by an enum of the chromosome names of `head`) and /metadata/rebin_map.  gd_gw_contact_matrix writes it from the
// stored maps, gd_interphase --ensemble-matrix from the maps of its replicas as they are dumped.
inline void write_gw_matrix(std::string const &output, trajectory const &head, rebinning const &rb, std::vector<int32_t> const &matrix)
{
    h5::hid file(H5Fcreate(output.c_str(), H5F_ACC_TRUNC, H5P_DEFAULT, H5P_DEFAULT));
    h5::check(file >= 0, "cannot create " + output);
    h5::hid names(H5Tenum_create(H5T_STD_I32LE));
    for (auto const &kv : head.keys) {
        int32_t const v = (int32_t)kv.second;
        H5Tenum_insert(names, kv.first.c_str(), &v);
    }
    cli::put_dataset(file, "/metadata/chromosome_ranges", rb.binned.data(), {rb.binned.size() / 2, 2}, 4, names, names, nullptr);
    cli::put(file, "/metadata/rebin_map", rb.map.data(), {rb.map.size()}, nullptr);
    cli::filters f;
    f.scaleoffset_kind = H5Z_SO_INT;
    f.scaleoffset_factor = H5Z_SO_INT_MINBITS_DEFAULT;      // scaleoffset=0: integer scale-offset is lossless
    cli::put(file, "/contact_matrix", matrix.data(), {rb.n_bins, rb.n_bins}, &f);
    H5Fflush(file, H5F_SCOPE_GLOBAL);
}

inline void run_gw(options const &o)
{
    cli::stopwatch sw;
    request meta_only;
    meta_only.how = frames::none;
    trajectory const head = load(o.inputs[0], meta_only);
    rebinning const rb = rebin(head, o.rebin_rate);
    request rq;
    rq.how = frames::by_slice;
    rq.o = &o;
    prefetcher pf(o.inputs, rq);
    sw.read += sw.lap();
    device dev;
    open(dev);
    int32_t id = -1;
    cli::check(gd_cmap_add_binned(dev.h, rb.map.data(), (uint32_t)rb.map.size(), rb.n_bins, &id));
    std::fputs("Loading: ", stderr);
    for (std::size_t k = 0; k < o.inputs.size(); k++) {
        trajectory const t = pf.take();
        sw.read += sw.lap();
        cli::check(gd_cmap_accumulate(dev.h, t.rows.data(), t.rows.size() / 3));
        sw.compute += sw.lap();
        if (k % 10 == 0) std::fprintf(stderr, "%zu", k);
        std::fputc('.', stderr);
        std::fflush(stderr);
    }
    std::fputs(" DONE\n", stderr);
    auto const matrix = fetch(dev, id);
    sw.compute += sw.lap();
    write_gw_matrix(o.output, head, rb, matrix);
    sw.write += sw.lap();
    sw.report("gd_gw_contact_matrix");
    dev.report("gd_gw_contact_matrix");
}

// ---- power_law

// fit_power_law (power_law.py:85-92) in closed form: the weighted least-squares slope of log y on log x, weights 1 / x, over
// x > 0 and y > 0, for the slice [beg, end) of the profile
inline double fit_exponent(std::vector<int32_t> const &profile, std::size_t beg, std::size_t end)
{
    end = std::min(end, profile.size());
    double sw = 0, sx = 0, sy = 0;
    std::size_t points = 0;
    for (std::size_t x = std::max<std::size_t>(beg, 1); x < end; x++) {
        if (profile[x] <= 0) continue;
        double const w = 1.0 / (double)x;
        sw += w;
        sx += w * std::log((double)x);
        sy += w * std::log((double)profile[x]);
        points++;
    }
    if (points == 0) throw std::runtime_error("no contact at separations " + std::to_string(beg) + " to " + std::to_string(end) + ": nothing to fit");
    double const xm = sx / sw, ym = sy / sw;
    double var = 0, cov = 0;
    for (std::size_t x = std::max<std::size_t>(beg, 1); x < end; x++) {
        if (profile[x] <= 0) continue;
        double const w = 1.0 / (double)x, dx = std::log((double)x) - xm;
        var += w * dx * dx;
        cov += w * dx * (std::log((double)profile[x]) - ym);
    }
    return var > 0 ? cov / var : 0.0;
}

inline void run_power_law(options const &o)
{
    cli::stopwatch sw;
    request rq;
    rq.how = frames::last_with_map;
    rq.o = &o;
    rq.types = true;
    prefetcher pf(o.inputs, rq);
    device dev;
    for (std::size_t k = 0; k < o.inputs.size(); k++) {
        trajectory t = pf.take();
        sw.read += sw.lap();
        if (t.maps == 0) throw std::runtime_error(o.inputs[k] + ": no interphase frame has a contact_map");      // UnboundLocalError
        // compute_contact_profile: chain ids, -1 (the reference's NaN) outside every chromosome
        std::vector<int32_t> chain(t.n_particles, -1);
        uint32_t longest = 0;
        for (std::size_t c = 0; c + 1 < t.ranges.size(); c += 2) {
            h5::check((std::size_t)t.ranges[c + 1] <= t.n_particles, o.inputs[k] + ": a chromosome ends beyond particle_types");
            for (int b = t.ranges[c]; b < t.ranges[c + 1]; b++) chain[(std::size_t)b] = (int32_t)(c / 2);
            longest = std::max(longest, (uint32_t)(t.ranges[c + 1] - t.ranges[c]));
        }
        open(dev);
        cli::check(gd_cmap_clear(dev.h));
        int32_t id = -1;
        cli::check(gd_cmap_add_separation_profile(dev.h, chain.data(), (uint32_t)chain.size(), longest, &id));
        cli::check(gd_cmap_accumulate(dev.h, t.rows.data(), t.rows.size() / 3));
        auto const profile = fetch(dev, id);
        double const near = fit_exponent(profile, 3, 20), mid = fit_exponent(profile, 20, 100), far = fit_exponent(profile, 100, 1500);
        sw.compute += sw.lap();
        std::printf("%g\t%g\t%g\n", near, mid, far);
        std::fflush(stdout);
        sw.write += sw.lap();
    }
    sw.report("gd_power_law");
    dev.report("gd_power_law");
}

// status 0, 1 (error: <what>) or 2 (usage)
inline int main(program p, int argc, char **argv)
{
    options o;
    return cli::run(usage(p), name_of(p), "error:", [&](std::string &err) { return parse(p, argc, argv, o, err); },
                    [&] { return o.dry_run && (print_plan(p, o), true); }, [&] {
        if (p == program::gw_contact_matrix) run_gw(o);
        else if (p == program::power_law) run_power_law(o);
        else run_by_step(p, o);
        return 0;
    });
}

}  // namespace cmap
}  // namespace gd
