// gd_structure_factor -- structure factors and scattering functions of trajectories on the device (include/gdyn_sq.h): for every
// trajectory file, the sums behind the partial structure factors S_ab(q) and the collective intermediate scattering function
// F_ab(q, tau) of the labels of its beads, and on request its self part F_s(q, tau) and the amplitudes of every frame, over the frames
// of a phase.  The reference has no such analysis.  Per input sample, under /sq/<name>/<sample>/ of the output file:
//   q (Q, 3) float64, q_norm (Q) float64, label_names (K) fixed-length strings, label_sizes (K) uint64, lags (L) uint32
//   sum_re, sum_im (L, K, K, Q) float64, count (L) uint64               F_ab(q, tau) = sum_re / (count * n); lag 0: S_ab(q)
//   --self:       self_cos, self_sin (L, K, Q) float64, self_count (L, K) uint64            F_s(q, tau) = self_cos / self_count
//   --amplitudes: cos_sum, sin_sum (F, K, Q) float64                    rho_a(q, f) = cos_sum - i sin_sum
//   gd_structure_factor [--name PHASE] (--box Lx,Ly,Lz --n-max M | --magnitudes q1,q2,... --directions D) [--groups all|types]
//                       [--frames FIRST:COUNT] [--lags a,b,...|--log-lags K] [--self] [--origin-stride k] [--amplitudes] [--dry-run]
//                       outfile trajfiles...
// --name: the phase whose frames are read (/snapshots/PHASE, default interphase) and the name of the output group.  Vectors: the
// lattice vectors 2 pi n / L of a periodic box with 0 < max |n_k| <= M, one of every pair +-n, in lexicographic order (sq.py,
// Sq.lattice_vectors), or D Fibonacci-sphere directions times every magnitude (Sq.sphere_vectors).  Labels: all beads (default)
// or the values of /metadata/particle_types, as gd_dcorr reads them.  Lags: lag 0 always, then those of --lags or --log-lags (K
// values spaced geometrically up to the longest lag of the window); without either, lag 0 alone.  --dry-run prints the plan and, for
// every trajectory file given, the lags it resolves to and the shape of every dataset; no device is used and nothing is written.
#include "../../include/gdyn_sq.h"
#include "gd_lag_cli.hpp"

using namespace gd::lagcli;

namespace {

constexpr double TWO_PI = 6.283185307179586;
constexpr double GOLDEN_ANGLE = 2.399963229728653;      // pi (3 - sqrt 5)
constexpr long MAX_N_MAX = 63;                            // ((2 M + 1)^3 - 1) / 2 <= GD_SQ_MAX_VECTORS

struct options {
    std::string name = "interphase", groups = "all";
    lag_option lags;
    bool has_lags = false, has_box = false, has_n_max = false, has_magnitudes = false, has_directions = false, has_frames = false;
    bool self = false, amplitudes = false, dry_run = false;
    double box[3] = {0, 0, 0};
    long n_max = 0, directions = 0, origin_stride = 1, first_frame = 0, n_frames = 0;
    std::vector<double> magnitudes;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

bool parse_magnitudes(std::string const &v, std::vector<double> &out)
{
    out.clear();
    std::size_t at = 0;
    while (at <= v.size()) {
        auto const comma = std::min(v.find(',', at), v.size());
        double m = 0;
        if (!gd::cli::parse_float(v.substr(at, comma - at), m) || !(m >= 0) || !std::isfinite(m)) return false;
        out.push_back(m);
        at = comma + 1;
    }
    return !out.empty();
}

bool parse_frames(std::string const &v, long &first, long &count)
{
    auto const colon = v.find(':');
    return colon != std::string::npos && gd::cli::parse_int(v.substr(0, colon), first) && gd::cli::parse_int(v.substr(colon + 1), count) && first >= 0 &&
           count >= 1 && first <= 0xffffffffl && count <= 0xffffffffl;
}

int parse(int argc, char **argv, options &o, std::string &err)
{
    using gd::cli::kind;
    static gd::cli::table const options = {{"--dry-run", kind::flag}, {"--self", kind::flag}, {"--amplitudes", kind::flag}, {"--name", kind::value},
                                           {"--box", kind::value}, {"--n-max", kind::value}, {"--magnitudes", kind::value}, {"--directions", kind::value},
                                           {"--groups", kind::value}, {"--frames", kind::value}, {"--lags", kind::value}, {"--log-lags", kind::value},
                                           {"--origin-stride", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--dry-run") return o.dry_run = true, std::string();
        if (key == "--self") return o.self = true, std::string();
        if (key == "--amplitudes") return o.amplitudes = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--box") return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
        if (key == "--n-max") return o.has_n_max = true, gd::cli::to_int(v, o.n_max, nullptr, 1, MAX_N_MAX);
        if (key == "--magnitudes") return gd::cli::valid_if(o.has_magnitudes = parse_magnitudes(v, o.magnitudes), v);
        if (key == "--directions") return o.has_directions = true, gd::cli::to_int(v, o.directions, nullptr, 1, GD_SQ_MAX_VECTORS);
        if (key == "--groups") return gd::cli::valid_if((o.groups = v) == "all" || v == "types", v);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--lags" || key == "--log-lags") return o.has_lags = true, lags_or_count(o.lags, key == "--lags", v);
        return gd::cli::to_int(v, o.origin_stride, nullptr, 1, 0xffffffffl);
    }, pos);
    if (!err.empty()) return 2;
    bool const lattice = o.has_box || o.has_n_max, sphere = o.has_magnitudes || o.has_directions;
    if (lattice && sphere) err = "argument --magnitudes: not allowed with argument --box";
    else if (!lattice && !sphere) err = "one of the arguments --box --magnitudes is required";
    else if (lattice && !o.has_n_max) err = "argument --box: requires argument --n-max";
    else if (lattice && !o.has_box) err = "argument --n-max: requires argument --box";
    else if (sphere && !o.has_directions) err = "argument --magnitudes: requires argument --directions";
    else if (sphere && !o.has_magnitudes) err = "argument --directions: requires argument --magnitudes";
    else if (sphere && (uint64_t)o.magnitudes.size() * (uint64_t)o.directions > GD_SQ_MAX_VECTORS)
        err = "argument --directions: more than " + std::to_string(GD_SQ_MAX_VECTORS) + " vectors";
    if (!err.empty()) return 2;
    return gd::flow::take_files(pos, o.dry_run, o.outfile, o.trajfiles, err);
}

// Sq.lattice_vectors: q_k = (TWO_PI * n_k) / L_k of the integer triples with 0 < max |n_k| <= n_max whose first non-zero component is
// positive, in lexicographic order
std::vector<double> lattice_vectors(double const box[3], long n_max)
{
    std::vector<double> q;
    for (long nx = -n_max; nx <= n_max; nx++)
        for (long ny = -n_max; ny <= n_max; ny++)
            for (long nz = -n_max; nz <= n_max; nz++) {
                long const first = nx ? nx : ny ? ny : nz;
                if (first <= 0) continue;
                long const n[3] = {nx, ny, nz};
                for (int k = 0; k < 3; k++) q.push_back((TWO_PI * (double)n[k]) / box[k]);
            }
    return q;
}

// Sq.sphere_vectors: direction i of D has z = 1 - (2 i + 1) / D and the azimuth i times the golden angle, normalised
std::vector<double> sphere_vectors(std::vector<double> const &magnitudes, long D)
{
    std::vector<double> u(3 * (std::size_t)D), q;
    for (long i = 0; i < D; i++) {
        double const z = 1.0 - (2.0 * (double)i + 1.0) / (double)D, r = std::sqrt(1.0 - z * z);
        double const v[3] = {r * std::cos(GOLDEN_ANGLE * (double)i), r * std::sin(GOLDEN_ANGLE * (double)i), z};
        double const norm = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        for (int k = 0; k < 3; k++) u[3 * (std::size_t)i + k] = v[k] / norm;
    }
    for (double m : magnitudes)
        for (double c : u) q.push_back(m * c);
    return q;
}

struct plan {      // the window and the lags of one trajectory file
    uint32_t first_frame = 0, n_frames = 0;
    std::vector<uint32_t> lags;      // lag 0 first
};

plan make_plan(options const &o, std::string const &path, uint32_t F)
{
    plan p;
    p.first_frame = o.has_frames ? (uint32_t)o.first_frame : 0;
    p.n_frames = o.has_frames ? (uint32_t)o.n_frames : F;
    gd::h5::check((uint64_t)p.first_frame + p.n_frames <= F, path + ": --frames " + std::to_string(p.first_frame) + ":" + std::to_string(p.n_frames) + " of " +
                                                                 std::to_string(F) + " frames");
    p.lags.push_back(0);
    if (o.has_lags)
        for (uint32_t lag : resolve(o.lags, p.n_frames - 1)) {
            gd::h5::check(lag < p.n_frames, path + ": lag " + std::to_string(lag) + " of a window of " + std::to_string(p.n_frames) + " frames");
            p.lags.push_back(lag);
        }
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
    char const *usage = "usage: gd_structure_factor [--name PHASE] (--box Lx,Ly,Lz --n-max M | --magnitudes q1,q2,... --directions D) [--groups all|types] "
                        "[--frames FIRST:COUNT] [--lags a,b,...|--log-lags K] [--self] [--origin-stride k] [--amplitudes] [--dry-run] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_structure_factor", "gd_structure_factor: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        std::vector<double> const q = o.has_box ? lattice_vectors(o.box, o.n_max) : sphere_vectors(o.magnitudes, o.directions);
        std::size_t const Q = q.size() / 3;
        if (o.dry_run) {
            std::string const vectors = o.has_box ? "lattice box " + join_doubles({o.box[0], o.box[1], o.box[2]}) + " n_max " + std::to_string(o.n_max)
                                                  : "sphere magnitudes " + join_doubles(o.magnitudes) + " directions " + std::to_string(o.directions);
            std::printf("name\t%s\nvectors\t%s (%zu)\ngroups\t%s\nframes\t%s\nlags\t%s\nself\t%s\norigin stride\t%ld\namplitudes\t%s\n", o.name.c_str(), vectors.c_str(),
                        Q, o.groups.c_str(), o.has_frames ? (std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames)).c_str() : "all",
                        o.has_lags ? ("0," + describe(o.lags)).c_str() : "0", o.self ? "yes" : "no", o.origin_stride, o.amplitudes ? "yes" : "no");
            for (auto const &path : o.trajfiles) {
                uint32_t F = 0, N = 0;
                gd::flow::load_history(path, F, N, o.name);
                layout const l = read_layout(path, o.name, o.groups, N);
                plan const p = make_plan(o, path, F);
                std::string const sample = gd::cli::sample_name(path);
                std::size_t const K = l.group_names.size(), L = p.lags.size();
                std::printf("sample\t%s\tframes %u\tbeads %u\tlabels %zu\tvectors %zu\n", sample.c_str(), F, N, K, Q);
                std::printf("lags\t%s\t%s\n", sample.c_str(), join(p.lags).c_str());
                std::printf("shapes\t%s\tq (%zu, 3)\tsum_re (%zu, %zu, %zu, %zu)\tcount (%zu)", sample.c_str(), Q, L, K, K, Q, L);
                if (o.self) std::printf("\tself_cos (%zu, %zu, %zu)\tself_count (%zu, %zu)", L, K, Q, L, K);
                if (o.amplitudes) std::printf("\tcos_sum (%u, %zu, %zu)", p.n_frames, K, Q);
                std::printf("\n");
            }
            return 0;
        }
        gd::cli::handle<gd_sq, gd_sq_destroy> dev;
        dev.open([](gd_sq **h) { gd_sq_desc const d{0, 0}; return gd_sq_create(&d, h); });
        gd::cli::check(gd_sq_set_vectors(dev.h, q.data(), (uint32_t)Q));
        std::vector<double> q_norm(Q);
        for (std::size_t k = 0; k < Q; k++) q_norm[k] = std::sqrt((q[3 * k] * q[3 * k] + q[3 * k + 1] * q[3 * k + 1]) + q[3 * k + 2] * q[3 * k + 2]);
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, o.groups, N);
            plan const p = make_plan(o, path, F);
            sw.read += sw.lap();
            std::size_t const K = l.group_names.size(), L = p.lags.size();
            std::vector<uint64_t> label_sizes(K, 0);
            for (uint32_t i = 0; i < N; i++) label_sizes[l.group.empty() ? 0 : (std::size_t)l.group[i]]++;
            gd::cli::check(gd_sq_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_sq_set_labels(dev.h, l.group.empty() ? nullptr : l.group.data(), (uint32_t)K));
            std::vector<double> re(L * K * K * Q), im(L * K * K * Q), self_cos, self_sin, amp_cos, amp_sin;
            std::vector<uint64_t> count(L), self_count;
            gd::cli::check(gd_sq_collective(dev.h, p.first_frame, p.n_frames, p.lags.data(), (uint32_t)L, (uint32_t)o.origin_stride, re.data(), im.data(), count.data()));
            if (o.self) {
                self_cos.resize(L * K * Q), self_sin.resize(L * K * Q), self_count.resize(L * K);
                gd::cli::check(gd_sq_self(dev.h, p.first_frame, p.n_frames, p.lags.data(), (uint32_t)L, (uint32_t)o.origin_stride, self_cos.data(), self_sin.data(),
                                          self_count.data()));
            }
            if (o.amplitudes) {
                amp_cos.resize((std::size_t)p.n_frames * K * Q), amp_sin.resize((std::size_t)p.n_frames * K * Q);
                gd::cli::check(gd_sq_amplitudes(dev.h, p.first_frame, p.n_frames, amp_cos.data(), amp_sin.data()));
            }
            sw.compute += sw.lap();
            gd::h5::hid group(gd::cli::require_group(out, "/sq/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            hsize_t const nq = Q, nk = K, nl = L;
            gd::cli::put(group, "q", q.data(), {nq, 3}, nullptr);
            gd::cli::put(group, "q_norm", q_norm.data(), {nq}, nullptr);
            gd::cli::put(group, "label_sizes", label_sizes.data(), {nk}, nullptr);
            gd::cli::put(group, "lags", p.lags.data(), {nl}, nullptr);
            gd::cli::put(group, "sum_re", re.data(), {nl, nk, nk, nq}, &f);
            gd::cli::put(group, "sum_im", im.data(), {nl, nk, nk, nq}, &f);
            gd::cli::put(group, "count", count.data(), {nl}, nullptr);
            for (char const *name : {"self_cos", "self_sin", "self_count", "cos_sum", "sin_sum"}) gd::h5::unlink_if_present(group, name);      // of an earlier run
            if (o.self) {
                gd::cli::put(group, "self_cos", self_cos.data(), {nl, nk, nq}, &f);
                gd::cli::put(group, "self_sin", self_sin.data(), {nl, nk, nq}, &f);
                gd::cli::put(group, "self_count", self_count.data(), {nl, nk}, nullptr);
            }
            if (o.amplitudes) {
                gd::cli::put(group, "cos_sum", amp_cos.data(), {p.n_frames, nk, nq}, &f);
                gd::cli::put(group, "sin_sum", amp_sin.data(), {p.n_frames, nk, nq}, &f);
            }
            gd::h5::unlink_if_present(group, "label_names");
            gd::h5::write_fixed_string_list(group, "label_names", l.group_names);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_structure_factor");
        return 0;
    });
}
