// gd_dcorr -- the spatial correlation of bead displacements of trajectories on the device (include/gdyn_dcorr.h): for every
// trajectory file and lag, per pair class and distance bin, the number of pairs and the sum of D_i . D_j over all origins of a
// phase.  The reference has no such analysis.  Per input sample, under /dcorr/<name>/<sample>/ of the output file:
//   lags (L) uint32, bin_edges (n_bins + 1) float64, class_names (P) fixed-length strings, scale_bits (L) int32
//   count (L, P, n_bins) uint64, sum (L, P, n_bins) float64            <D_i . D_j>(r) = sum / count
//   self_count (L, K) uint64, self_sum (L, K) float64                   <|D|^2> of a label = self_sum / self_count
//   with --per-origin also per_origin/lag_<lag>/{count, sum, self_count, self_sum}: the raw tables (origins first), the sums
//   int64 in units of 2^-scale_bits
// The library's per-origin integer sums are added over the origins as 128-bit integers and written as float64 of sum / 2^scale_bits.
//   gd_dcorr [--name PHASE] --lags a,b,...|--log-lags K --bin-width W --max-distance R [--groups all|types] [--split-chains]
//            [--origin-stride k] [--box Lx,Ly,Lz] [--per-origin] [--dry-run] outfile trajfiles...
// --name: the phase whose frames are read (/snapshots/PHASE; default interphase) and the name of the output group.  Labels: all
// beads (default) or the values of /metadata/particle_types.  --split-chains: every class is split into same chain / different
// chain by the phase's chromosome_ranges, else the file's (beads of no range share one more chain).  --box: periodic; else open.
// Without --lags: --log-lags 16.  --dry-run prints the plan and, for every trajectory file given, the lags it resolves to; no
// device is used and nothing is written.
#include "../../include/gdyn_dcorr.h"
#include "gd_lag_cli.hpp"

using namespace gd::lagcli;

namespace {

struct options {
    std::string name = "interphase", groups = "all";
    lag_option lags;
    double bin_width = 0, max_distance = 0, box[3] = {0, 0, 0};
    bool has_box = false, split_chains = false, per_origin = false, dry_run = false;
    long origin_stride = 1;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--split-chains", kind::flag}, {"--per-origin", kind::flag}, {"--name", kind::value},
                                           {"--lags", kind::value}, {"--log-lags", kind::value}, {"--groups", kind::value}, {"--bin-width", kind::value},
                                           {"--max-distance", kind::value}, {"--origin-stride", kind::value}, {"--box", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--split-chains") return o.split_chains = true, std::string();
        if (key == "--per-origin") return o.per_origin = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--groups") return gd::cli::valid_if((o.groups = v) == "all" || v == "types", v);
        if (key == "--lags" || key == "--log-lags") return lags_or_count(o.lags, key == "--lags", v);
        if (key == "--bin-width") return gd::cli::to_float(v, o.bin_width);
        if (key == "--max-distance") return gd::cli::to_float(v, o.max_distance);
        if (key == "--origin-stride") return gd::cli::to_int(v, o.origin_stride, nullptr, 1, 0xffffffffl);
        return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
    }, pos);
    if (!err.empty()) return 2;
    if (!gd_dcorr_bins(o.bin_width, o.max_distance)) {
        err = "--bin-width and --max-distance are required, positive and finite, with at most " + std::to_string(GD_DCORR_MAX_BINS) + " bins";
        return 2;
    }
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

// the chain of every bead: the index of its range; beads of no range share the index one past the last range
std::vector<uint32_t> chain_ids(layout const &l, uint32_t N)
{
    uint32_t const C = (uint32_t)(l.chains.size() / 2);
    std::vector<uint32_t> id(N, C);
    for (uint32_t c = 0; c < C; c++)
        for (uint32_t i = l.chains[2 * c]; i < l.chains[2 * c + 1]; i++) id[i] = c;
    return id;
}

std::vector<std::string> class_names(std::vector<std::string> const &labels, bool split)
{
    std::vector<std::string> out;
    for (std::size_t a = 0; a < labels.size(); a++)
        for (std::size_t b = a; b < labels.size(); b++) {
            std::string const pair = labels[a] + "-" + labels[b];
            if (split) {
                out.push_back(pair + "/same");
                out.push_back(pair + "/different");
            } else {
                out.push_back(pair);
            }
        }
    return out;
}

// out[c] += in[o, c] over the origins, as 128-bit integers; then float64 of sum / 2^S
template <typename T>
void total(std::vector<T> const &in, std::size_t origins, std::size_t cells, std::vector<__int128> &acc)
{
    acc.assign(cells, 0);
    for (std::size_t o = 0; o < origins; o++)
        for (std::size_t c = 0; c < cells; c++) acc[c] += (__int128)in[o * cells + c];
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_dcorr [--name PHASE] --lags a,b,...|--log-lags K --bin-width W --max-distance R [--groups all|types] [--split-chains] "
                        "[--origin-stride k] [--box Lx,Ly,Lz] [--per-origin] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_dcorr", "gd_dcorr: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        uint32_t const n_bins = gd_dcorr_bins(o.bin_width, o.max_distance);
        if (o.dry_run) {
            std::printf("name\t%s\ngroups\t%s\nsplit chains\t%s\nlags\t%s\nbins\t%u of %s up to %s\norigin stride\t%ld\nbox\t%s\n", o.name.c_str(),
                        o.groups.c_str(), o.split_chains ? "yes" : "no", describe(o.lags).c_str(), n_bins, gd::cli::py_float(o.bin_width).c_str(),
                        gd::cli::py_float(o.max_distance).c_str(), o.origin_stride,
                        o.has_box ? (gd::cli::py_float(o.box[0]) + "," + gd::cli::py_float(o.box[1]) + "," + gd::cli::py_float(o.box[2])).c_str() : "open");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, o.groups, N);
                std::string const sample = gd::cli::sample_name(path);
                std::printf("sample\t%s\tframes %u\tbeads %u\tchains %zu\tlabels %zu\n", sample.c_str(), F, N, l.chains.size() / 2, l.group_names.size());
                std::printf("lags\t%s\t%s\n", sample.c_str(), join(resolve(o.lags, F - 1)).c_str());
            }
            return 0;
        }
        gd::cli::handle<gd_dcorr, gd_dcorr_destroy> dev;
        dev.open([](gd_dcorr **h) { gd_dcorr_desc const d{0, 0}; return gd_dcorr_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, o.groups, N);
            auto const lags = resolve(o.lags, F - 1);
            sw.read += sw.lap();
            uint32_t const K = (uint32_t)l.group_names.size();
            gd::cli::check(gd_dcorr_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_dcorr_set_labels(dev.h, l.group.empty() ? nullptr : l.group.data(), K));
            std::vector<uint32_t> const chains = o.split_chains ? chain_ids(l, N) : std::vector<uint32_t>();
            gd::cli::check(gd_dcorr_set_chains(dev.h, o.split_chains ? chains.data() : nullptr));
            uint32_t const P = gd_dcorr_classes(dev.h);
            std::size_t const cells = (std::size_t)P * n_bins, L = lags.size();
            std::vector<uint64_t> count_total(L * cells), self_count_total(L * K);
            std::vector<double> sum_total(L * cells), self_sum_total(L * K);
            std::vector<int32_t> scale(L);
            gd::h5::hid group(gd::cli::require_group(out, "/dcorr/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            for (std::size_t k = 0; k < L; k++) {
                uint32_t const O = gd_dcorr_origins(dev.h, lags[k], 0, 0, (uint32_t)o.origin_stride);
                std::vector<uint64_t> count((std::size_t)O * cells), self_count((std::size_t)O * K);
                std::vector<int64_t> sum((std::size_t)O * cells), self_sum((std::size_t)O * K);
                gd::cli::check(gd_dcorr_pairs(dev.h, lags[k], 0, 0, (uint32_t)o.origin_stride, o.has_box ? o.box : nullptr, o.bin_width, o.max_distance, 0,
                                              &scale[k], count.data(), sum.data(), self_count.data(), self_sum.data()));
                sw.compute += sw.lap();
                double const unit = std::ldexp(1.0, scale[k]);
                std::vector<__int128> acc;
                total(count, O, cells, acc);
                for (std::size_t c = 0; c < cells; c++) count_total[k * cells + c] = (uint64_t)acc[c];
                total(sum, O, cells, acc);
                for (std::size_t c = 0; c < cells; c++) sum_total[k * cells + c] = (double)acc[c] / unit;
                total(self_count, O, K, acc);
                for (std::size_t c = 0; c < K; c++) self_count_total[k * K + c] = (uint64_t)acc[c];
                total(self_sum, O, K, acc);
                for (std::size_t c = 0; c < K; c++) self_sum_total[k * K + c] = (double)acc[c] / unit;
                if (o.per_origin) {
                    std::string const at = "per_origin/lag_" + std::to_string(lags[k]) + "/";
                    gd::cli::put(group, at + "count", count.data(), {O, P, n_bins}, &f);
                    gd::cli::put(group, at + "sum", sum.data(), {O, P, n_bins}, &f);
                    gd::cli::put(group, at + "self_count", self_count.data(), {O, K}, &f);
                    gd::cli::put(group, at + "self_sum", self_sum.data(), {O, K}, &f);
                    sw.write += sw.lap();
                }
            }
            std::vector<double> edges(n_bins + 1);
            for (uint32_t b = 0; b <= n_bins; b++) edges[b] = std::min((double)b * o.bin_width, o.max_distance);
            gd::cli::put(group, "lags", lags.data(), {L}, nullptr);
            gd::cli::put(group, "bin_edges", edges.data(), {n_bins + 1}, nullptr);
            gd::cli::put(group, "scale_bits", scale.data(), {L}, nullptr);
            gd::cli::put(group, "count", count_total.data(), {L, P, n_bins}, &f);
            gd::cli::put(group, "sum", sum_total.data(), {L, P, n_bins}, &f);
            gd::cli::put(group, "self_count", self_count_total.data(), {L, K}, &f);
            gd::cli::put(group, "self_sum", self_sum_total.data(), {L, K}, &f);
            gd::h5::unlink_if_present(group, "class_names");
            gd::h5::write_fixed_string_list(group, "class_names", class_names(l.group_names, o.split_chains));
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_dcorr");
        return 0;
    });
}
