// gd_distance_map -- distance and contact-frequency maps of trajectories on the device (include/gdyn_dmap.h): for every trajectory
// file, the sums behind the mean and rms spatial distance of every pair of bins and the number of bead pairs closer than each
// threshold, over the frames of a phase.  The reference has no such analysis.  Per input sample, under /dmap/<name>/<sample>/ of the
// output file, with S the selected bins:
//   bins (S, 2) uint32, bin_chain (S) uint32, chain_names (C) fixed-length strings, thresholds (T) float64,
//   sum1, sum2 (S, S) float64, hits (T, S, S) uint64, count (S, S) uint64       mean distance = sum1 / count, frequency = hits / count
//   gd_distance_map [--name PHASE] [--rebin-rate K] [--by-chain] [--chains a,b,...] [--thresholds t1,t2,...] [--frames FIRST:COUNT]
//                   [--box Lx,Ly,Lz] [--dry-run] outfile trajfiles...
// --name: the phase whose frames are read (/snapshots/PHASE, default interphase) and the name of the output group.  Chains: the
// phase's chromosome_ranges, else the file's, else one chain of all beads, as gd_msd reads them.  Bins: K consecutive beads of a chain
// (default 1; the last bin of a chain is shorter, no bin spans two chains: tests/dmap_restatement.py, bins_from_chains), or with
// --by-chain every non-empty chain as one bin.  --chains restricts rows and columns to the bins of the chains named.  --dry-run prints
// the plan and, for every trajectory file given, its shape and bins; no device is used.
#include "../../include/gdyn_dmap.h"
#include "gd_bins_cli.hpp"

using namespace gd::lagcli;
using namespace gd::binscli;

namespace {

struct options : bin_options {
    std::string name = "interphase";
    bool has_box = false, has_frames = false, dry_run = false;
    std::vector<double> thresholds;
    long first_frame = 0, n_frames = 0;
    double box[3] = {0, 0, 0};
    std::string outfile;
    std::vector<std::string> trajfiles;
};

bool parse_thresholds(std::string const &v, std::vector<double> &out)
{
    out.clear();
    for (auto const &s : split(v)) {
        double t = 0;
        if (!gd::cli::parse_float(s, t) || !(t > 0) || !std::isfinite(t)) return false;
        out.push_back(t);
    }
    return out.size() <= GD_DMAP_MAX_THRESHOLDS;
}

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--by-chain", kind::flag}, {"--name", kind::value}, {"--rebin-rate", kind::value},
                                           {"--chains", kind::value}, {"--thresholds", kind::value}, {"--frames", kind::value}, {"--box", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--by-chain") return o.by_chain = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--rebin-rate") return gd::cli::to_int(v, o.rate, nullptr, 1, 1l << 28);
        if (key == "--chains") return gd::cli::valid_if(parse_chains(v, o.chains), v);
        if (key == "--thresholds") return gd::cli::valid_if(parse_thresholds(v, o.thresholds), v);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
    }, pos);
    if (!err.empty()) return 2;
    if (!(err = conflict(o)).empty()) return 2;
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

struct plan : bin_plan {
    uint32_t first_frame = 0, n_frames = 0;
};

plan make_plan(options const &o, layout const &l, std::string const &path, uint32_t F)
{
    plan p;
    plan_bins(o, l, path, p);
    p.first_frame = o.has_frames ? (uint32_t)o.first_frame : 0;
    p.n_frames = o.has_frames ? (uint32_t)o.n_frames : F;
    gd::h5::check((uint64_t)p.first_frame + p.n_frames <= F, path + ": --frames " + std::to_string(p.first_frame) + ":" + std::to_string(p.n_frames) + " of " +
                                                                 std::to_string(F) + " frames");
    return p;
}

std::string join_doubles(std::vector<double> const &v)
{
    std::string s;
    for (std::size_t k = 0; k < v.size(); k++) s += (k ? "," : "") + gd::cli::py_float(v[k]);
    return s;
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_distance_map [--name PHASE] [--rebin-rate K] [--by-chain] [--chains a,b,...] [--thresholds t1,t2,...] [--frames FIRST:COUNT] "
                        "[--box Lx,Ly,Lz] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_distance_map", "gd_distance_map: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        if (o.dry_run) {
            std::string const chains = join_names(o.chains);
            std::printf("name\t%s\nbins\t%s\nchains\t%s\nthresholds\t%s\nframes\t%s\nbox\t%s\n", o.name.c_str(),
                        o.by_chain ? "by chain" : ("rate " + std::to_string(o.rate)).c_str(), o.chains.empty() ? "all" : chains.c_str(),
                        o.thresholds.empty() ? "none" : join_doubles(o.thresholds).c_str(),
                        o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all",
                        o.has_box ? join_doubles({o.box[0], o.box[1], o.box[2]}).c_str() : "open");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, "all", N);
                plan const p = make_plan(o, l, path, F);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tbins %zu\tselected %zu\n", gd::cli::sample_name(path).c_str(), F, N, l.chains.size() / 2,
                            p.bin_chain.size(), p.selected.size());
            }
            return 0;
        }
        gd::cli::handle<gd_dmap, gd_dmap_destroy> dev;
        dev.open([](gd_dmap **h) { gd_dmap_desc const d{0, 0}; return gd_dmap_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, "all", N);
            plan const p = make_plan(o, l, path, F);
            sw.read += sw.lap();
            std::size_t const S = p.selected.size(), T = o.thresholds.size();
            std::vector<double> sum1(S * S), sum2(S * S);
            std::vector<uint64_t> hits(T * S * S), count(S * S);
            gd::cli::check(gd_dmap_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_dmap_set_bins(dev.h, p.bins.data(), (uint32_t)p.bin_chain.size()));
            auto const runs = runs_of(p.selected);
            std::vector<double> r1, r2;
            std::vector<uint64_t> rh, rc;
            for (run const &a : runs)
                for (run const &b : runs) {      // one rectangle per pair of runs of selected bins: a cell does not know its region
                    std::size_t const cells = (std::size_t)a.n * b.n;
                    r1.resize(cells), r2.resize(cells), rc.resize(cells), rh.resize(T * cells);
                    gd::cli::check(gd_dmap_map(dev.h, a.first, a.n, b.first, b.n, p.first_frame, p.n_frames, o.has_box ? o.box : nullptr, o.thresholds.data(),
                                               (uint32_t)T, r1.data(), r2.data(), T ? rh.data() : nullptr, rc.data()));
                    for (std::size_t i = 0; i < a.n; i++)
                        for (std::size_t j = 0; j < b.n; j++) {
                            std::size_t const to = (a.at + i) * S + b.at + j, from = i * b.n + j;
                            sum1[to] = r1[from];
                            sum2[to] = r2[from];
                            count[to] = rc[from];
                            for (std::size_t t = 0; t < T; t++) hits[t * S * S + to] = rh[t * cells + from];
                        }
                }
            sw.compute += sw.lap();
            gd::h5::hid group(gd::cli::require_group(out, "/dmap/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const s = S, t = T;
            put_selected(group, p, l.chain_names, f);
            gd::cli::put(group, "thresholds", o.thresholds.data(), {t}, nullptr);
            gd::cli::put(group, "sum1", sum1.data(), {s, s}, &f);
            gd::cli::put(group, "sum2", sum2.data(), {s, s}, &f);
            gd::cli::put(group, "hits", hits.data(), {t, s, s}, &f);
            gd::cli::put(group, "count", count.data(), {s, s}, &f);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_distance_map");
        return 0;
    });
}
