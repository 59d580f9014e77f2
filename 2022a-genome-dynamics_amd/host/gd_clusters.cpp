// gd_clusters -- the connected clusters of trajectories on the device (include/gdyn_cluster.h): for every trajectory file and
// frame of a phase, the connected components of the graph whose edges are the pairs of beads closer than a distance.  The
// reference has no such analysis.  Per input sample, under /clusters/<name>/<sample>/ of the output file:
//   frames (F) uint32                        the frames analysed, as indices into the phase's snapshots
//   summary (F, 4) uint64                    selected beads, clusters, the largest cluster, the sum of s^2 over the clusters
//   histogram (F, K) uint64                  clusters of size b + 1; the last bin: those of K beads and more
//   root (F, N) int32, with --roots          the smallest bead index of every bead's cluster, -1 for a bead that takes no part
//   label_names (K) fixed-length strings, and the arguments as attributes of the group: distance, links, link_mask, box (absent: open),
//   frame_stride, size_bins
//   gd_clusters [--name PHASE] --distance D [--groups all|types] [--links all|same|a-b,c-d,...] [--frames FIRST:COUNT]
//               [--frame-stride k] [--box Lx,Ly,Lz] [--size-bins K] [--roots] outfile trajfiles...
// --name: the phase whose frames are read (/snapshots/PHASE; default interphase) and the name of the output group.  Labels: all
// beads (default) or the values of /metadata/particle_types, as gd_dcorr reads them.  --links: the label pairs that may link, by
// label index: all of them (default), each label with itself only, or a list.  --box: periodic; else open.
#include "../../include/gdyn_cluster.h"
#include "gd_lag_cli.hpp"

using namespace gd::lagcli;

namespace {

struct options {
    std::string name = "interphase", groups = "all", links = "all";
    std::vector<std::pair<long, long>> pairs;      // of --links a-b,...
    double distance = 0, box[3] = {0, 0, 0};
    bool has_distance = false, has_box = false, has_frames = false, roots = false;
    long first_frame = 0, n_frames = 0, frame_stride = 1, size_bins = 64;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

// all | same | a-b,c-d,... with label indices below GD_CLUSTER_MAX_LABELS
bool parse_links(std::string const &v, std::vector<std::pair<long, long>> &out)
{
    out.clear();
    if (v == "all" || v == "same") return true;
    std::size_t at = 0;
    while (at <= v.size()) {
        auto const comma = std::min(v.find(',', at), v.size());
        std::string const item = v.substr(at, comma - at);
        auto const dash = item.find('-');
        long a = 0, b = 0;
        if (dash == std::string::npos || !gd::cli::parse_int(item.substr(0, dash), a) || !gd::cli::parse_int(item.substr(dash + 1), b) || a < 0 || b < 0 ||
            a >= GD_CLUSTER_MAX_LABELS || b >= GD_CLUSTER_MAX_LABELS)
            return false;
        out.emplace_back(a, b);
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
    static gd::cli::table const options = {{"--roots", kind::flag}, {"--name", kind::value}, {"--distance", kind::value}, {"--groups", kind::value},
                                           {"--links", kind::value}, {"--frames", kind::value}, {"--frame-stride", kind::value}, {"--box", kind::value},
                                           {"--size-bins", kind::value}};
    std::vector<std::string> pos;
    err = gd::cli::scan(argc, argv, options, [&o](std::string const &key, std::string const &v) {
        if (key == "--roots") return o.roots = true, std::string();
        if (key == "--name") return phase_name(v, o.name);
        if (key == "--distance") return gd::cli::valid_if(o.has_distance = gd::cli::parse_float(v, o.distance) && o.distance > 0 && std::isfinite(o.distance), v);
        if (key == "--groups") return gd::cli::valid_if((o.groups = v) == "all" || v == "types", v);
        if (key == "--links") return gd::cli::valid_if(parse_links(o.links = v, o.pairs), v);
        if (key == "--frames") return gd::cli::valid_if(o.has_frames = parse_frames(v, o.first_frame, o.n_frames), v);
        if (key == "--frame-stride") return gd::cli::to_int(v, o.frame_stride, nullptr, 1, 0xffffffffl);
        if (key == "--size-bins") return gd::cli::to_int(v, o.size_bins, nullptr, 1, (long)GD_CLUSTER_MAX_SIZE_BINS);
        return gd::cli::valid_if(o.has_box = parse_box(v, o.box), v);
    }, pos);
    if (!err.empty()) return 2;
    if (!o.has_distance) {
        err = "the following arguments are required: --distance";
        return 2;
    }
    return gd::flow::take_files(pos, false, o.outfile, o.trajfiles, err);
}

// the mask of --links for K labels (cluster.py: link_mask)
uint64_t link_mask(options const &o, uint32_t K)
{
    auto const cls = [K](uint64_t a, uint64_t b) { return a * K - a * (a ? a - 1 : 0) / 2 + (b - a); };
    uint64_t mask = 0;
    if (o.links == "all") return (1ull << (K * (K + 1) / 2)) - 1;
    if (o.links == "same") {
        for (uint32_t a = 0; a < K; a++) mask |= 1ull << cls(a, a);
        return mask;
    }
    for (auto const &p : o.pairs) {
        gd::h5::check(p.first < (long)K && p.second < (long)K, "--links " + o.links + ": the beads have " + std::to_string(K) + " labels");
        mask |= 1ull << cls((uint64_t)std::min(p.first, p.second), (uint64_t)std::max(p.first, p.second));
    }
    return mask;
}

template <typename T>
void put_attribute(hid_t obj, char const *name, hid_t mem_type, hid_t file_type, T const *data, hsize_t count)
{
    if (H5Aexists(obj, name) > 0) H5Adelete(obj, name);
    gd::h5::hid space(count ? H5Screate_simple(1, &count, nullptr) : H5Screate(H5S_SCALAR));
    gd::h5::hid attr(H5Acreate2(obj, name, file_type, space, H5P_DEFAULT, H5P_DEFAULT));
    gd::h5::check(attr >= 0 && H5Awrite(attr, mem_type, data) >= 0, std::string("cannot write attribute ") + name);
}

void put_string_attribute(hid_t obj, char const *name, std::string const &value)
{
    if (H5Aexists(obj, name) > 0) H5Adelete(obj, name);
    gd::h5::hid type(gd::h5::vlen_string_type()), space(H5Screate(H5S_SCALAR));
    gd::h5::hid attr(H5Acreate2(obj, name, type, space, H5P_DEFAULT, H5P_DEFAULT));
    char const *p = value.c_str();
    gd::h5::check(attr >= 0 && H5Awrite(attr, type, &p) >= 0, std::string("cannot write attribute ") + name);
}

}  // namespace

int main(int argc, char **argv)
{
    options o;
    char const *usage = "usage: gd_clusters [--name PHASE] --distance D [--groups all|types] [--links all|same|a-b,c-d,...] [--frames FIRST:COUNT] "
                        "[--frame-stride k] [--box Lx,Ly,Lz] [--size-bins K] [--roots] outfile trajfiles ...\n";
    return gd::cli::run(usage, "gd_clusters", "gd_clusters: error:", [&](std::string &err) { return parse(argc, argv, o, err); }, gd::cli::no_plan, [&o] {
        gd::cli::handle<gd_cluster, gd_cluster_destroy> dev;
        dev.open([](gd_cluster **h) { gd_cluster_desc const d{0, 0}; return gd_cluster_create(&d, h); });
        gd::h5::hid out(gd::cli::open_output(o.outfile));
        gd::cli::stopwatch sw;
        uint32_t const stride = (uint32_t)o.frame_stride, nb = (uint32_t)o.size_bins;
        for (auto const &path : o.trajfiles) {
            uint32_t F = 0, N = 0;
            auto const hist = gd::flow::load_history(path, F, N, o.name);
            layout const l = read_layout(path, o.name, o.groups, N);
            uint32_t const first = o.has_frames ? (uint32_t)o.first_frame : 0;
            gd::h5::check(first < F && (!o.has_frames || (uint64_t)first + (uint64_t)(o.n_frames - 1) * stride < F),
                          path + ": --frames " + std::to_string(o.first_frame) + ":" + std::to_string(o.n_frames) + " with stride " + std::to_string(stride) + " of " +
                              std::to_string(F) + " frames");
            uint32_t const K = (uint32_t)l.group_names.size();
            gd::h5::check(K <= GD_CLUSTER_MAX_LABELS, path + ": " + std::to_string(K) + " particle types (at most " + std::to_string(GD_CLUSTER_MAX_LABELS) + ")");
            uint64_t const mask = link_mask(o, K);
            sw.read += sw.lap();
            gd::cli::check(gd_cluster_set_history(dev.h, hist.data(), F, N, 0));
            gd::cli::check(gd_cluster_set_labels(dev.h, l.group.empty() ? nullptr : l.group.data(), K));
            gd::cli::check(gd_cluster_set_links(dev.h, mask));
            uint32_t const count = gd_cluster_frames(dev.h, first, o.has_frames ? (uint32_t)o.n_frames : 0, stride);
            std::vector<uint32_t> frames(count);
            for (uint32_t k = 0; k < count; k++) frames[k] = first + k * stride;
            std::vector<uint64_t> summary((std::size_t)count * 4), histogram((std::size_t)count * nb);
            std::vector<int32_t> root(o.roots ? (std::size_t)count * N : 0);
            gd::cli::check(gd_cluster_components(dev.h, first, count, stride, o.has_box ? o.box : nullptr, o.distance, nb, o.roots ? root.data() : nullptr,
                                                 summary.data(), histogram.data()));
            sw.compute += sw.lap();
            gd::h5::hid group(gd::cli::require_group(out, "/clusters/" + o.name + "/" + gd::cli::sample_name(path)));
            gd::cli::filters const f;
            gd::cli::put(group, "frames", frames.data(), {count}, nullptr);
            gd::cli::put(group, "summary", summary.data(), {count, 4}, nullptr);
            gd::cli::put(group, "histogram", histogram.data(), {count, nb}, &f);
            gd::h5::unlink_if_present(group, "root");      // of an earlier run
            if (o.roots) gd::cli::put(group, "root", root.data(), {count, N}, &f);
            gd::h5::unlink_if_present(group, "label_names");
            gd::h5::write_fixed_string_list(group, "label_names", l.group_names);
            uint64_t const stride64 = stride, bins64 = nb;
            put_attribute(group, "distance", H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, &o.distance, 0);
            put_string_attribute(group, "links", o.links);
            put_attribute(group, "link_mask", H5T_NATIVE_UINT64, H5T_STD_U64LE, &mask, 0);
            put_attribute(group, "frame_stride", H5T_NATIVE_UINT64, H5T_STD_U64LE, &stride64, 0);
            put_attribute(group, "size_bins", H5T_NATIVE_UINT64, H5T_STD_U64LE, &bins64, 0);
            if (H5Aexists(group, "box") > 0) H5Adelete(group, "box");
            if (o.has_box) put_attribute(group, "box", H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE, o.box, 3);
            H5Fflush(out, H5F_SCOPE_GLOBAL);
            sw.write += sw.lap();
        }
        sw.report("gd_clusters");
        return 0;
    });
}
