// gd_covariance_map -- displacement covariance maps of trajectories on the device (include/gdyn_dcov.h): for every trajectory file, the
// sum behind the covariance of the displacements of every pair of bins over a lag, or with --fluctuation of their positions about the
// time mean, over the frames of a phase.  The reference has no such analysis.  Per input sample, under /dcov/<name>/<sample>/ of the
// output file, with S the selected bins and O the origins:
//   bins (S, 2) uint32, bin_chain (S) uint32, chain_names (C) fixed-length strings, lag (1) uint32 (0: fluctuation), origins (O) uint32
//   (the origin frames), remove_drift (1) uint32, sum (S, S) float64, count (S, S) uint64       mean covariance = sum / count
//   with --rows: rows (S, 3 O) float64, every selected bin's displacement series, column 3 k + axis
//   gd_covariance_map [--name PHASE] (--lag L | --fluctuation) [--frames FIRST:COUNT] [--origin-stride k] [--remove-drift] [--rebin-rate K]
//                     [--by-chain] [--chains a,b,...] [--rows] [--dry-run] outfile trajfiles...
// --name, the chains and the bin options (--rebin-rate, --by-chain, --chains) are gd_distance_map's (gd_bins_cli.hpp).  The origins are
// the frames FIRST + j k of the window whose frame L later lies in the window too; with --fluctuation, every k-th frame of the window.
// --remove-drift subtracts the mean displacement of the binned beads, column by column, before the product.  --dry-run prints the plan
// and, for every trajectory file given, its shape, bins and origins; no device is used.
#include "../../include/gdyn_dcov.h"
#include "gd_bins_cli.hpp"

using namespace gd::lagcli;
using namespace gd::binscli;

namespace {

struct options : bin_options {
    std::string name = "interphase";
    long lag = 0, stride = 1;
    bool has_lag = false, fluctuation = false, has_frames = false, remove_drift = false, rows = false, dry_run = false;
    long first_frame = 0, n_frames = 0;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--by-chain", kind::flag}, {"--fluctuation", kind::flag}, {"--remove-drift", kind::flag},
                                           {"--rows", kind::flag}, {"--name", kind::value}, {"--lag", kind::value}, {"--frames", kind::value},
                                           {"--origin-stride", kind::value}, {"--rebin-rate", kind::value}, {"--chains", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--by-chain") return o.by_chain = true, std::string();
        if (key == "--fluctuation") return o.fluctuation = true, std::string();
        if (key == "--remove-drift") return o.remove_drift = true, std::string();
        if (key == "--rows") return o.rows = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--lag") return o.has_lag = true, gd::cli::to_int(v, o.lag, nullptr, 1, 0xffffffffl);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--origin-stride") return gd::cli::to_int(v, o.stride, nullptr, 1, 0xffffffffl);
        if (key == "--rebin-rate") return gd::cli::to_int(v, o.rate, nullptr, 1, 1l << 28);
        return gd::cli::valid_if(parse_chains(v, o.chains), v);
    }, pos);
    if (!err.empty()) return 2;
    if (o.has_lag && o.fluctuation) { err = "argument --fluctuation: not allowed with argument --lag"; return 2; }
    if (!o.has_lag && !o.fluctuation) { err = "one of the arguments --lag --fluctuation is required"; return 2; }
    if (!(err = conflict(o)).empty()) return 2;
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

struct plan : bin_plan {
    uint32_t lag = 0, first_frame = 0, n_origins = 0;
};

plan make_plan(options const &o, layout const &l, std::string const &path, uint32_t F)
{
    plan p;
    plan_bins(o, l, path, p);
    p.lag = o.fluctuation ? 0 : (uint32_t)o.lag;
    p.first_frame = o.has_frames ? (uint32_t)o.first_frame : 0;
    uint64_t const n_frames = o.has_frames ? (uint64_t)o.n_frames : F;
    gd::h5::check(p.first_frame + n_frames <= F, path + ": --frames " + std::to_string(p.first_frame) + ":" + std::to_string(n_frames) + " of " +
                                                     std::to_string(F) + " frames");
    gd::h5::check(n_frames > p.lag, path + ": --lag " + std::to_string(p.lag) + " leaves no origin in " + std::to_string(n_frames) + " frames");
    p.n_origins = (uint32_t)((n_frames - p.lag - 1) / (uint64_t)o.stride + 1);
    return p;
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_covariance_map [--name PHASE] (--lag L | --fluctuation) [--frames FIRST:COUNT] [--origin-stride k] [--remove-drift] "
                        "[--rebin-rate K] [--by-chain] [--chains a,b,...] [--rows] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_covariance_map", "gd_covariance_map: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        if (o.dry_run) {
            std::string const chains = join_names(o.chains);
            std::printf("name\t%s\nmode\t%s\nbins\t%s\nchains\t%s\nframes\t%s\norigin stride\t%ld\nremove drift\t%s\nrows\t%s\n", o.name.c_str(),
                        o.fluctuation ? "fluctuation" : ("lag " + std::to_string(o.lag)).c_str(),
                        o.by_chain ? "by chain" : ("rate " + std::to_string(o.rate)).c_str(), o.chains.empty() ? "all" : chains.c_str(),
                        o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all", o.stride,
                        o.remove_drift ? "yes" : "no", o.rows ? "yes" : "no");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, "all", N);
                plan const p = make_plan(o, l, path, F);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tbins %zu\tselected %zu\torigins %u\n", gd::cli::sample_name(path).c_str(), F, N,
                            l.chains.size() / 2, p.bin_chain.size(), p.selected.size(), p.n_origins);
            }
            return 0;
        }
        gd::cli::handle<gd_dcov, gd_dcov_destroy> dev;
        dev.open([](gd_dcov **h) { gd_dcov_desc const d{0, 0}; return gd_dcov_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, "all", N);
            plan const p = make_plan(o, l, path, F);
            sw.read += sw.lap();
            std::size_t const S = p.selected.size();
            gd::cli::check(gd_dcov_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_dcov_set_bins(dev.h, p.bins.data(), (uint32_t)p.bin_chain.size()));
            gd::cli::check(gd_dcov_prepare(dev.h, p.lag, p.first_frame, (uint32_t)o.stride, p.n_origins, o.remove_drift));
            std::size_t const columns = gd_dcov_columns(dev.h);
            std::vector<double> sum(S * S), rows(o.rows ? S * columns : 0);
            std::vector<uint64_t> count(S * S);
            auto const runs = runs_of(p.selected);
            std::vector<double> rs;
            std::vector<uint64_t> rc;
            for (run const &a : runs) {
                if (o.rows) gd::cli::check(gd_dcov_rows(dev.h, a.first, a.n, rows.data() + a.at * columns));
                for (run const &b : runs) {      // one rectangle per pair of runs of selected bins: a cell does not know its rectangle
                    std::size_t const cells = (std::size_t)a.n * b.n;
                    rs.resize(cells), rc.resize(cells);
                    gd::cli::check(gd_dcov_map(dev.h, a.first, a.n, b.first, b.n, rs.data(), rc.data(), nullptr, nullptr));
                    for (std::size_t i = 0; i < a.n; i++)
                        for (std::size_t j = 0; j < b.n; j++) {
                            sum[(a.at + i) * S + b.at + j] = rs[i * b.n + j];
                            count[(a.at + i) * S + b.at + j] = rc[i * b.n + j];
                        }
                }
            }
            sw.compute += sw.lap();
            std::vector<uint32_t> origins(p.n_origins);
            for (uint32_t k = 0; k < p.n_origins; k++) origins[k] = p.first_frame + k * (uint32_t)o.stride;
            uint32_t const lag = p.lag, drift = o.remove_drift;
            gd::h5::hid group(gd::cli::require_group(out, "/dcov/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const s = S;
            put_selected(group, p, l.chain_names, f);
            gd::cli::put(group, "lag", &lag, {1}, nullptr);
            gd::cli::put(group, "remove_drift", &drift, {1}, nullptr);
            gd::cli::put(group, "origins", origins.data(), {(hsize_t)origins.size()}, &f);
            gd::cli::put(group, "sum", sum.data(), {s, s}, &f);
            gd::cli::put(group, "count", count.data(), {s, s}, &f);
            if (o.rows) gd::cli::put(group, "rows", rows.data(), {s, (hsize_t)columns}, &f);
            else gd::h5::unlink_if_present(group, "rows");      // of an earlier run with --rows
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_covariance_map");
        return 0;
    });
}
