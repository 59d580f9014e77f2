// gd_van_hove -- the van Hove functions of trajectories on the device (include/gdyn_vanhove.h): for every trajectory file and lag, the
// histogram of the displacements of single beads per label (the self part, with an axis mask: xy is a microscope's projection) and, with
// --distinct, the histogram of the distances from where a bead was to where the OTHER beads are a lag later, per ordered label pair.
// The reference has no such analysis.  Per input sample, under /vanhove/<name>/<sample>/ of the output file, with L the lags, K the
// labels, B the bins and O the origins:
//   lags (L) uint32, edges (B + 1) float64, origins (L) uint64: the origins that take part in a lag
//   self (L, K, B), below (L, K), above (L, K) uint64
//   with --per-origin:  self_per_origin (L, O, K, B) uint64
//   with --distinct:    distinct (L, K, K, B) uint64: [lag, label at the origin, label of the other, bin]; with --box also box (3) float64
//   gd_van_hove [--name PHASE] (--lags a,b,... | --log-lags K) (--edges e0,e1,... | --bin-width W --max-distance R |
//               --log-edges E0:E1:PER_DECADE) [--axes xyz|xy|x|...] [--groups all|types] [--frames FIRST:COUNT] [--origin-stride k]
//               [--per-origin] [--distinct [--box Lx,Ly,Lz]] [--dry-run] outfile trajfiles...
// --name, --lags, --log-lags, --groups and --box are gd_dcorr's (gd_lag_cli.hpp), --frames gd_distance_map's (gd_bins_cli.hpp).  The
// origins are the frames of the window FIRST .. FIRST + COUNT - 1 (default: all), every k-th; the partner of an origin may lie beyond
// the window.  Lags are in frames of the file, at most 32; without --lags: --log-lags 16.  The edges are those of vanhove.py:
// linear_edges(W, R) or log_edges(E0, E1, PER_DECADE).  A run without --per-origin, --distinct or --box removes what an earlier run
// left of them.  The divisions (densities, the overlap, chi_4) are the caller's (vanhove.py).  --dry-run prints the plan and, for every
// trajectory file given, its shape, labels, lags and origins; no device is used.
#include <cmath>

#include "../../include/gdyn_vanhove.h"
#include "gd_bins_cli.hpp"

using namespace gd::lagcli;
using namespace gd::binscli;

namespace {

struct options {
    std::string name = "interphase", groups = "all", axes = "xyz";
    lag_option lags;
    std::vector<double> edges;      // --edges
    double bin_width = 0, max_distance = 0, log_first = 0, log_last = 0, box[3] = {0, 0, 0};
    long per_decade = 0, origin_stride = 1, first_frame = 0, n_frames = 0;
    bool has_edges = false, has_width = false, has_max = false, has_log_edges = false, has_frames = false, has_box = false;
    bool per_origin = false, distinct = false, dry_run = false;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

// --edges e0,e1,...: 2 to GD_VANHOVE_MAX_BINS + 1 finite values, 0 <= e0 < e1 < ...
bool parse_edges(std::string const &v, std::vector<double> &out)
{
    out.clear();
    for (auto const &word : split(v)) {
        double e = 0;
        if (!gd::cli::parse_float(word, e) || !std::isfinite(e) || e < 0 || (!out.empty() && !(e > out.back()))) return false;
        out.push_back(e);
    }
    return out.size() >= 2 && out.size() <= GD_VANHOVE_MAX_BINS + 1;
}

// --log-edges E0:E1:PER_DECADE: 0 < E0 < E1, finite, PER_DECADE of at least 1
bool parse_log_edges(std::string const &v, double &first, double &last, long &per_decade)
{
    auto const a = v.find(':'), b = a == std::string::npos ? a : v.find(':', a + 1);
    return b != std::string::npos && gd::cli::parse_float(v.substr(0, a), first) && gd::cli::parse_float(v.substr(a + 1, b - a - 1), last) &&
           gd::cli::parse_int(v.substr(b + 1), per_decade) && first > 0 && first < last && std::isfinite(last) && per_decade >= 1 && per_decade <= 1000;
}

// --axes: each of x, y, z at most once, at least one
unsigned axes_mask(std::string const &v)
{
    unsigned mask = 0;
    for (char c : v) {
        unsigned const bit = c == 'x' ? 1u : c == 'y' ? 2u : c == 'z' ? 4u : 0u;
        if (!bit || (mask & bit)) return 0;
        mask |= bit;
    }
    return mask;
}

// the edges of a run (vanhove.py: linear_edges, log_edges); empty: more than GD_VANHOVE_MAX_BINS bins
std::vector<double> make_edges(options const &o)
{
    if (o.has_edges) return o.edges;
    double const n = o.has_log_edges ? std::ceil(std::log10(o.log_last / o.log_first) * (double)o.per_decade - 1e-9) : std::ceil(o.max_distance / o.bin_width);
    if (!(n >= 1) || n > GD_VANHOVE_MAX_BINS) return {};
    std::vector<double> e((std::size_t)n + 1);
    for (std::size_t k = 0; k < e.size(); k++) e[k] = o.has_log_edges ? o.log_first * std::pow(10.0, (double)k / (double)o.per_decade) : (double)k * o.bin_width;
    return e;
}

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--per-origin", kind::flag}, {"--distinct", kind::flag}, {"--name", kind::value},
                                           {"--lags", kind::value}, {"--log-lags", kind::value}, {"--edges", kind::value}, {"--bin-width", kind::value},
                                           {"--max-distance", kind::value}, {"--log-edges", kind::value}, {"--axes", kind::value}, {"--groups", kind::value},
                                           {"--frames", kind::value}, {"--origin-stride", kind::value}, {"--box", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--per-origin") return o.per_origin = true, std::string();
        if (key == "--distinct") return o.distinct = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--lags" || key == "--log-lags") return lags_or_count(o.lags, key == "--lags", v);
        if (key == "--edges") return gd::cli::valid_if(o.has_edges = parse_edges(v, o.edges), v);
        if (key == "--bin-width") return o.has_width = true, gd::cli::to_float(v, o.bin_width);
        if (key == "--max-distance") return o.has_max = true, gd::cli::to_float(v, o.max_distance);
        if (key == "--log-edges") return gd::cli::valid_if(o.has_log_edges = parse_log_edges(v, o.log_first, o.log_last, o.per_decade), v);
        if (key == "--axes") return gd::cli::valid_if(axes_mask(o.axes = v) != 0, v);
        if (key == "--groups") return gd::cli::valid_if((o.groups = v) == "all" || v == "types", v);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--origin-stride") return gd::cli::to_int(v, o.origin_stride, nullptr, 1, 0xffffffffl);
        return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
    }, pos);
    if (!err.empty()) return 2;
    bool const linear = o.has_width || o.has_max;
    if ((int)o.has_edges + (int)linear + (int)o.has_log_edges != 1) {
        err = "one of the arguments --edges, --bin-width with --max-distance, --log-edges is required";
        return 2;
    }
    if (linear && !(o.has_width && o.has_max && o.bin_width > 0 && o.max_distance > 0 && std::isfinite(o.bin_width) && std::isfinite(o.max_distance))) {
        err = "--bin-width and --max-distance go together, positive and finite";
        return 2;
    }
    if (make_edges(o).empty()) {
        err = "the edges make more than " + std::to_string(GD_VANHOVE_MAX_BINS) + " bins";
        return 2;
    }
    if (o.lags.explicit_list && o.lags.list.size() > GD_VANHOVE_MAX_LAGS) {
        err = "argument --lags: at most " + std::to_string(GD_VANHOVE_MAX_LAGS) + " lags";
        return 2;
    }
    if (o.has_box && !o.distinct) {
        err = "argument --box: only with --distinct";
        return 2;
    }
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

struct plan {
    uint32_t first = 0, count = 0;      // the origins first + j stride, j < count
    std::vector<uint32_t> lags;
};

plan make_plan(options const &o, std::string const &path, uint32_t F)
{
    plan p;
    p.first = o.has_frames ? (uint32_t)o.first_frame : 0;
    uint64_t const n_frames = o.has_frames ? (uint64_t)o.n_frames : F;
    gd::h5::check(p.first + n_frames <= F, path + ": --frames " + std::to_string(p.first) + ":" + std::to_string(n_frames) + " of " + std::to_string(F) + " frames");
    p.count = (uint32_t)((n_frames - 1) / (uint64_t)o.origin_stride + 1);
    p.lags = resolve(o.lags, F - 1);
    gd::h5::check(!p.lags.empty() && p.lags.size() <= GD_VANHOVE_MAX_LAGS,
                  path + ": " + std::to_string(p.lags.size()) + " lags of " + std::to_string(F) + " frames, 1 to " + std::to_string(GD_VANHOVE_MAX_LAGS) + " are served");
    return p;
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_van_hove [--name PHASE] (--lags a,b,... | --log-lags K) (--edges e0,e1,... | --bin-width W --max-distance R | "
                        "--log-edges E0:E1:PER_DECADE) [--axes xyz|xy|x|...] [--groups all|types] [--frames FIRST:COUNT] [--origin-stride k] [--per-origin] "
                        "[--distinct [--box Lx,Ly,Lz]] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_van_hove", "gd_van_hove: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        std::vector<double> const edges = make_edges(o);
        std::size_t const B = edges.size() - 1;
        if (o.dry_run) {
            std::printf("name\t%s\ngroups\t%s\naxes\t%s\nlags\t%s\nbins\t%zu from %s to %s\nframes\t%s\norigin stride\t%ld\nper origin\t%s\ndistinct\t%s\nbox\t%s\n",
                        o.name.c_str(), o.groups.c_str(), o.axes.c_str(), describe(o.lags).c_str(), B, gd::cli::py_float(edges.front()).c_str(),
                        gd::cli::py_float(edges.back()).c_str(), o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all",
                        o.origin_stride, o.per_origin ? "yes" : "no", o.distinct ? "yes" : "no",
                        o.has_box ? (gd::cli::py_float(o.box[0]) + "," + gd::cli::py_float(o.box[1]) + "," + gd::cli::py_float(o.box[2])).c_str() : "open");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, o.groups, N);
                plan const p = make_plan(o, path, F);
                std::string const sample = gd::cli::sample_name(path);
                std::printf("sample\t%s\tframes %u\tbeads %u\tlabels %zu\torigins %u\n", sample.c_str(), F, N, l.group_names.size(), p.count);
                std::printf("lags\t%s\t%s\n", sample.c_str(), join(p.lags).c_str());
            }
            return 0;
        }
        gd::cli::handle<gd_vanhove, gd_vanhove_destroy> dev;
        dev.open([](gd_vanhove **h) { gd_vanhove_desc const d{0, 0, 0}; return gd_vanhove_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, o.groups, N);
            plan const p = make_plan(o, path, F);
            sw.read += sw.lap();
            std::size_t const K = l.group_names.size(), L = p.lags.size(), O = p.count;
            gd::cli::check(gd_vanhove_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_vanhove_set_labels(dev.h, l.group.empty() ? nullptr : l.group.data(), (uint32_t)K));
            gd_vanhove_spec const spec{p.lags.data(), (uint32_t)L, edges.data(), (uint32_t)B, p.first, (uint32_t)o.origin_stride, p.count};
            std::vector<uint64_t> counts(L * K * B), below(L * K), above(L * K), origins(L), per_origin(o.per_origin ? L * O * K * B : 0), distinct(o.distinct ? L * K * K * B : 0);
            gd_vanhove_self_out const to{counts.data(), below.data(), above.data(), o.per_origin ? per_origin.data() : nullptr, origins.data()};
            gd::cli::check(gd_vanhove_self(dev.h, &spec, axes_mask(o.axes), &to));
            if (o.distinct) gd::cli::check(gd_vanhove_distinct(dev.h, &spec, o.has_box ? o.box : nullptr, distinct.data(), nullptr));
            sw.compute += sw.lap();
            gd::h5::hid group(gd::cli::require_group(out, "/vanhove/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const n_lags = L, k = K, b = B, n_origins = O;
            gd::cli::put(group, "lags", p.lags.data(), {n_lags}, nullptr);
            gd::cli::put(group, "edges", edges.data(), {b + 1}, nullptr);
            gd::cli::put(group, "origins", origins.data(), {n_lags}, nullptr);
            gd::cli::put(group, "self", counts.data(), {n_lags, k, b}, &f);
            gd::cli::put(group, "below", below.data(), {n_lags, k}, &f);
            gd::cli::put(group, "above", above.data(), {n_lags, k}, &f);
            for (char const *name : {"self_per_origin", "distinct", "box"}) gd::h5::unlink_if_present(group, name);      // of an earlier run
            if (o.per_origin) gd::cli::put(group, "self_per_origin", per_origin.data(), {n_lags, n_origins, k, b}, &f);
            if (o.distinct) gd::cli::put(group, "distinct", distinct.data(), {n_lags, k, k, b}, &f);
            if (o.has_box) gd::cli::put(group, "box", o.box, {3}, nullptr);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_van_hove");
        return 0;
    });
}
