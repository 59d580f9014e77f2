// gd_dwell_times -- contact dwell times and the contact autocorrelation of trajectories on the device (include/gdyn_dwell.h): for every
// trajectory file and every separation s, the runs of the contact state of all pairs (i, i + s) inside one selected chain over the
// selected frames of a phase, by state (0 apart, 1 in contact), kind (0 complete, 1 left-censored, 2 right-censored, 3 both) and length
// bin, the sums of their lengths, and with --lags the products c_k c_{k+lag}.  The reference has no such analysis.  Per input sample,
// under /dwell/<name>/<sample>/ of the output file, with S the separations, B the bins, L the lags and K the selected frames:
//   separations (S), edges (B + 1), frames (K) uint32, contact (2) float64: r_on, r_off
//   runs (S, 2, 4, B), outside (S, 2, 4), length_sum (S, 2, 4), pairs (S) uint64
//   with --lags:  lags (L) uint32, hits (S, L) uint64
//   gd_dwell_times [--name PHASE] [--chains a,b,...] [--frames FIRST:COUNT] [--frame-stride k] --contact R_ON[:R_OFF]
//                  --separations s1,s2,... [--edges e0,e1,... | --log-edges PER_OCTAVE] [--lags l1,...] [--box Lx,Ly,Lz]
//                  [--dry-run] outfile trajfiles...
// --name, --chains and --frames are gd_distance_map's (gd_bins_cli.hpp), --box gd_dcorr's (gd_lag_cli.hpp).  Run lengths and lags are
// counted in selected frames, FIRST + j k of the window.  Without --edges the edges grow by 2^(1 / PER_OCTAVE) from 1 past the number
// of selected frames (dwell.py: Dwell.log_edges; --log-edges 1 when neither is given).  A run without --lags removes what an earlier
// run left of them.  The divisions (mean dwell time, autocorrelation, survival) are the caller's (dwell.py).  --dry-run prints the plan
// and, for every trajectory file given, its shape, chains, frames and bins; no device is used.
#include <cmath>

#include "../../include/gdyn_dwell.h"
#include "gd_bins_cli.hpp"

using namespace gd::lagcli;
using namespace gd::binscli;

namespace {

struct options {
    std::string name = "interphase";
    std::vector<std::string> chains;
    long stride = 1, per_octave = 1;
    bool has_frames = false, has_contact = false, has_edges = false, has_log_edges = false, has_box = false, dry_run = false;
    long first_frame = 0, n_frames = 0;
    double r_on = 0, r_off = 0, box[3] = {0, 0, 0};
    std::vector<uint32_t> separations, edges, lags;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

// a,b,...: 1 to `most` integers of at least `least`; ascending: each larger than the one before
bool parse_numbers(std::string const &v, std::vector<uint32_t> &out, long least, std::size_t most, bool ascending)
{
    out.clear();
    for (auto const &word : split(v)) {
        long x = 0;
        if (!gd::cli::parse_int(word, x) || x < least || x > 0xffffffffl || (ascending && !out.empty() && x <= (long)out.back())) return false;
        out.push_back((uint32_t)x);
    }
    return out.size() <= most;
}

// --contact R_ON[:R_OFF]: 0 < R_ON <= R_OFF, finite
bool parse_contact(std::string const &v, double &r_on, double &r_off)
{
    auto const colon = v.find(':');
    if (!gd::cli::parse_float(v.substr(0, colon), r_on)) return false;
    r_off = r_on;
    if (colon != std::string::npos && !gd::cli::parse_float(v.substr(colon + 1), r_off)) return false;
    return std::isfinite(r_on) && std::isfinite(r_off) && r_on > 0 && r_on <= r_off;
}

// Dwell.log_edges of dwell.py
std::vector<uint32_t> log_edges(uint32_t max_length, long per_octave)
{
    std::vector<uint32_t> out;
    for (long k = 0; out.empty() || out.back() <= max_length; k++) {
        uint32_t const e = (uint32_t)std::floor(std::pow(2.0, (double)k / (double)per_octave) + 1e-9);
        if (out.empty() || e > out.back()) out.push_back(e);
    }
    return out;
}

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--name", kind::value}, {"--chains", kind::value}, {"--frames", kind::value},
                                           {"--frame-stride", kind::value}, {"--contact", kind::value}, {"--separations", kind::value}, {"--edges", kind::value},
                                           {"--log-edges", kind::value}, {"--lags", kind::value}, {"--box", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--chains") return gd::cli::valid_if(parse_chains(v, o.chains), v);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--frame-stride") return gd::cli::to_int(v, o.stride, nullptr, 1, 0xffffffffl);
        if (key == "--contact") return gd::cli::valid_if(o.has_contact = parse_contact(v, o.r_on, o.r_off), v);
        if (key == "--separations") return gd::cli::valid_if(parse_numbers(v, o.separations, 1, GD_DWELL_MAX_SEPARATIONS, false), v);
        if (key == "--edges") return o.has_edges = true, gd::cli::valid_if(parse_numbers(v, o.edges, 1, GD_DWELL_MAX_BINS + 1, true) && o.edges.size() >= 2, v);
        if (key == "--log-edges") return o.has_log_edges = true, gd::cli::to_int(v, o.per_octave, nullptr, 1, 64);
        if (key == "--lags") return gd::cli::valid_if(parse_numbers(v, o.lags, 0, GD_DWELL_MAX_LAGS, false), v);
        return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
    }, pos);
    if (!err.empty()) return 2;
    if (o.has_edges && o.has_log_edges) { err = "argument --log-edges: not allowed with argument --edges"; return 2; }
    std::string missing = o.has_contact ? "" : "--contact";
    if (o.separations.empty()) missing += std::string(missing.empty() ? "" : ", ") + "--separations";
    if (!missing.empty()) { err = "the following arguments are required: " + missing; return 2; }
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

struct plan {
    uint32_t first_frame = 0, n_selected = 0;
    std::vector<uint32_t> chains, edges;      // the selected chains (., 2); the edges of this sample
    std::size_t n_chains = 0;                 // of the file
};

plan make_plan(options const &o, layout const &l, std::string const &path, uint32_t F)
{
    plan p;
    bin_options by_chain;
    by_chain.by_chain = true;
    by_chain.chains = o.chains;
    bin_plan b;
    plan_bins(by_chain, l, path, b);
    for (uint32_t s : b.selected) {
        p.chains.push_back(b.bins[2 * (std::size_t)s]);
        p.chains.push_back(b.bins[2 * (std::size_t)s + 1]);
    }
    p.n_chains = l.chains.size() / 2;
    p.first_frame = o.has_frames ? (uint32_t)o.first_frame : 0;
    uint64_t const n_frames = o.has_frames ? (uint64_t)o.n_frames : F;
    gd::h5::check(p.first_frame + n_frames <= F, path + ": --frames " + std::to_string(p.first_frame) + ":" + std::to_string(n_frames) + " of " +
                                                     std::to_string(F) + " frames");
    p.n_selected = (uint32_t)((n_frames - 1) / (uint64_t)o.stride + 1);
    p.edges = o.has_edges ? o.edges : log_edges(p.n_selected, o.per_octave);
    gd::h5::check(p.edges.size() <= GD_DWELL_MAX_BINS + 1, path + ": --log-edges " + std::to_string(o.per_octave) + " makes " + std::to_string(p.edges.size() - 1) +
                                                               " bins of " + std::to_string(p.n_selected) + " frames, at most " +
                                                               std::to_string(GD_DWELL_MAX_BINS) + " are served");
    return p;
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_dwell_times [--name PHASE] [--chains a,b,...] [--frames FIRST:COUNT] [--frame-stride k] --contact R_ON[:R_OFF] "
                        "--separations s1,s2,... [--edges e0,e1,... | --log-edges PER_OCTAVE] [--lags l1,...] [--box Lx,Ly,Lz] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_dwell_times", "gd_dwell_times: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        if (o.dry_run) {
            std::string const chains = join_names(o.chains), separations = join(o.separations), edges = join(o.edges), lags = join(o.lags);
            std::printf("name\t%s\nchains\t%s\nframes\t%s\nframe stride\t%ld\ncontact\t%s:%s\nseparations\t%s\nedges\t%s\nlags\t%s\nbox\t%s\n", o.name.c_str(),
                        o.chains.empty() ? "all" : chains.c_str(), o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all",
                        o.stride, gd::cli::py_float(o.r_on).c_str(), gd::cli::py_float(o.r_off).c_str(), separations.c_str(),
                        o.has_edges ? edges.c_str() : ("log " + std::to_string(o.per_octave)).c_str(), o.lags.empty() ? "none" : lags.c_str(),
                        o.has_box ? (gd::cli::py_float(o.box[0]) + "," + gd::cli::py_float(o.box[1]) + "," + gd::cli::py_float(o.box[2])).c_str() : "none");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, "all", N);
                plan const p = make_plan(o, l, path, F);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tselected %zu\tframes selected %u\tbins %zu\n", gd::cli::sample_name(path).c_str(), F, N,
                            p.n_chains, p.chains.size() / 2, p.n_selected, p.edges.size() - 1);
            }
            return 0;
        }
        gd::cli::handle<gd_dwell, gd_dwell_destroy> dev;
        dev.open([](gd_dwell **h) { gd_dwell_desc const d{0, 0}; return gd_dwell_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, "all", N);
            plan const p = make_plan(o, l, path, F);
            sw.read += sw.lap();
            std::size_t const S = o.separations.size(), B = p.edges.size() - 1, L = o.lags.size(), K = p.n_selected;
            gd::cli::check(gd_dwell_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_dwell_set_chains(dev.h, p.chains.data(), (uint32_t)(p.chains.size() / 2)));
            std::vector<uint64_t> runs(S * 8 * B), outside(S * 8), length_sum(S * 8), hits(S * L), pairs(S);
            gd_dwell_rule const rule{o.r_on, o.r_off, o.has_box ? o.box : nullptr, p.first_frame, (uint32_t)o.stride, p.n_selected};
            gd_dwell_spec const spec{p.edges.data(), (uint32_t)B, L ? o.lags.data() : nullptr, (uint32_t)L};
            gd_dwell_out const to{runs.data(), outside.data(), length_sum.data(), L ? hits.data() : nullptr, pairs.data()};
            gd::cli::check(gd_dwell_separations(dev.h, o.separations.data(), (uint32_t)S, &rule, &spec, &to));
            sw.compute += sw.lap();
            std::vector<uint32_t> frames(K);
            for (uint32_t k = 0; k < K; k++) frames[k] = p.first_frame + k * (uint32_t)o.stride;
            double const contact[2] = {o.r_on, o.r_off};
            gd::h5::hid group(gd::cli::require_group(out, "/dwell/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const s = S, b = B, n_lags = L, k = K;
            gd::cli::put(group, "separations", o.separations.data(), {s}, &f);
            gd::cli::put(group, "edges", p.edges.data(), {b + 1}, &f);
            gd::cli::put(group, "frames", frames.data(), {k}, &f);
            gd::cli::put(group, "contact", contact, {2}, &f);
            gd::cli::put(group, "runs", runs.data(), {s, 2, 4, b}, &f);
            gd::cli::put(group, "outside", outside.data(), {s, 2, 4}, &f);
            gd::cli::put(group, "length_sum", length_sum.data(), {s, 2, 4}, &f);
            gd::cli::put(group, "pairs", pairs.data(), {s}, &f);
            for (char const *name : {"lags", "hits"}) gd::h5::unlink_if_present(group, name);      // of an earlier run
            if (L) {
                gd::cli::put(group, "lags", o.lags.data(), {n_lags}, &f);
                gd::cli::put(group, "hits", hits.data(), {s, n_lags}, &f);
            }
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_dwell_times");
        return 0;
    });
}
