// gd_lamina_cli.hpp -- gd_analyze_lamina: the command line of the reference's analyze_lamina (scripts/analyze_lamina,
// 5-sim-genome/src/analyze_lamina/__main__.py), the inputs of command.py (interphase positions and the wall_semiaxes of
// each snapshot's context, the metadata of the first trajectory) and the datasets of its output file.  The arithmetic is
// libgdyn's (include/gdyn_lamina.h); the HDF5 helpers are the programs' shared ones (gd_cli_util.hpp).
#pragma once
#include <future>
#include <memory>

#include <json.hpp>   // nlohmann/json single header

#include "../../include/gdyn_lamina.h"
#include "gd_cli_util.hpp"

namespace gd {
namespace lamina {

struct options {
    std::string command;              // "distance" or "contact"
    std::string name = "uniform";
    bool has_contact_distance = false;
    double contact_distance = 0;
    bool dry_run = false;
    std::string outfile;
    std::vector<std::string> trajfiles;
};

inline const char *usage()
{
    return "usage: gd_analyze_lamina distance [--dry-run] outfile trajfiles ...\n"
           "       gd_analyze_lamina contact [--name NAME] --contact-distance D [--dry-run] outfile\n";
}

// argparse's conventions: "--opt value" or "--opt=value"; 0 or 2 with a message
inline int parse(int argc, char **argv, options &o, std::string &err)
{
    using cli::kind;
    static cli::table const before_contact = {{"--dry-run", kind::flag}},
                            after_contact = {{"--dry-run", kind::flag}, {"--name", kind::value}, {"--contact-distance", kind::value}};
    std::vector<std::string> pos;
    err = cli::scan_by(
        argc, argv, cli::shorts::exact, [](std::vector<std::string> const &p) -> cli::table const & { return !p.empty() && p[0] == "contact" ? after_contact : before_contact; },
        [&o](std::string const &key, std::string const &v) {
            if (key == "--dry-run") return o.dry_run = true, std::string();
            if (key == "--name") return o.name = v, std::string();
            return cli::valid_if(o.has_contact_distance = cli::parse_float(v, o.contact_distance), v, "float");
        },
        pos);
    if (!err.empty()) return 2;
    if (pos.empty()) { err = "the following arguments are required: command"; return 2; }
    o.command = pos[0];
    if (o.command != "distance" && o.command != "contact") {
        err = "argument command: invalid choice: '" + o.command + "' (choose from 'distance', 'contact')";
        return 2;
    }
    if (o.command == "contact") {
        // the reference's default None fails in `distances < None` after the file was opened: here it is a usage error
        if (!o.has_contact_distance) { err = "the following arguments are required: --contact-distance"; return 2; }
        if (pos.size() < 2) { err = "the following arguments are required: outfile"; return 2; }
        if (pos.size() > 2) { err = "unrecognized arguments: " + pos[2]; return 2; }
    } else if (pos.size() < 3) {
        err = "the following arguments are required: outfile, trajfiles";
        return 2;
    }
    o.outfile = pos[1];
    o.trajfiles.assign(pos.begin() + 2, pos.end());
    return 0;
}

inline void print_plan(options const &o)
{
    if (o.command == "distance") {
        std::printf("read\t%s\t/metadata/{config,particle_types,chromosome_ranges}\n", o.trajfiles[0].c_str());
        for (auto const &t : o.trajfiles) std::printf("read\t%s\t/snapshots/interphase/<step>/{positions,context}\n", t.c_str());
        std::printf("write\t%s\t/metadata/{simulation_config,particle_types,chromosome_ranges,chromosome_names}\n", o.outfile.c_str());
        for (auto const &t : o.trajfiles) std::printf("write\t%s\t/distance/%s\n", o.outfile.c_str(), cli::sample_name(t).c_str());
    } else {
        std::printf("contact_distance\t%s\n", cli::py_float(o.contact_distance).c_str());
        std::printf("read\t%s\t/distance/<key>\n", o.outfile.c_str());
        std::printf("write\t%s\t/contact/%s/<key>\n", o.outfile.c_str(), o.name.c_str());
        std::printf("write\t%s\t/average_contact/%s\n", o.outfile.c_str(), o.name.c_str());
    }
}

using device = cli::handle<gd_lamina, gd_lamina_destroy>;

inline void open(device &dev)
{
    dev.open([](gd_lamina **h) { gd_lamina_desc const d{0, 0}; return gd_lamina_create(&d, h); });
}

struct history {
    uint32_t frames = 0, beads = 0;
    std::vector<float> xyz;            // (F, N, 3)
    std::vector<double> semiaxes;      // (F, 3): wall_semiaxes of each snapshot's context
};

// analyze_distances_history's reads: the steps of /snapshots/interphase/.steps in stored order
inline history load_history(std::string const &path)
{
    history out;
    h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    h5::check(file >= 0, "cannot open " + path);
    h5::hid phase(H5Gopen2(file, "/snapshots/interphase", H5P_DEFAULT));
    h5::check(phase >= 0, path + ": no /snapshots/interphase");
    auto const steps = h5::read_string_list(phase, ".steps");
    for (auto const &s : steps) {
        h5::hid snap(H5Gopen2(phase, s.c_str(), H5P_DEFAULT));
        h5::check(snap >= 0, path + ": missing snapshot " + s);
        auto const context = nlohmann::json::parse(h5::read_string(snap, "context"));
        std::vector<double> const semi = context.at("wall_semiaxes");
        h5::check(semi.size() == 3, path + ": wall_semiaxes of snapshot " + s + " has not three values");
        std::size_t n = 0;
        auto const x = h5::read_array<float>(snap, "positions", 3, H5T_NATIVE_FLOAT, &n);
        if (out.frames == 0) out.beads = (uint32_t)n;
        h5::check(n == out.beads, path + ": snapshots disagree on the number of beads");      // np.array of ragged rows
        out.xyz.insert(out.xyz.end(), x.begin(), x.end());
        out.semiaxes.insert(out.semiaxes.end(), semi.begin(), semi.end());
        out.frames++;
    }
    return out;
}

// analyze_distance's metadata: copied from the first trajectory
inline void copy_metadata(std::string const &path, hid_t output)
{
    h5::hid file(H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT));
    h5::check(file >= 0, "cannot open " + path);
    h5::hid meta(H5Gopen2(file, "/metadata", H5P_DEFAULT));
    h5::check(meta >= 0, path + ": no /metadata");
    std::string const config = h5::read_string(meta, "config");
    // particle_types: the values with their enum type
    h5::hid types(H5Dopen2(meta, "particle_types", H5P_DEFAULT));
    h5::check(types >= 0, path + ": missing dataset metadata/particle_types");
    h5::hid ttype(H5Dget_type(types)), tspace(H5Dget_space(types));
    hssize_t const nt = H5Sget_simple_extent_npoints(tspace);
    std::vector<unsigned char> tdata((std::size_t)std::max<hssize_t>(nt, 0) * H5Tget_size(ttype));
    if (nt > 0) h5::check(H5Dread(types, ttype, H5S_ALL, H5S_ALL, H5P_DEFAULT, tdata.data()) >= 0, "cannot read particle_types");
    // chromosome_ranges and the names in the order of its keys attribute (name -> row)
    std::size_t rows = 0;
    auto const ranges = h5::read_array<int>(meta, "chromosome_ranges", 2, H5T_NATIVE_INT, &rows);
    h5::hid rds(H5Dopen2(meta, "chromosome_ranges", H5P_DEFAULT)), attr(H5Aopen(rds, "keys", H5P_DEFAULT));
    h5::check(attr >= 0, path + ": chromosome_ranges has no 'keys' attribute");
    auto const keys = nlohmann::json::parse(h5::read_string_from(attr, true));
    std::vector<std::string> names(rows);
    for (auto it = keys.begin(); it != keys.end(); ++it) names.at(it.value().get<std::size_t>()) = it.key();

    h5::hid out(cli::require_group(output, "/metadata"));
    h5::write_string(out, "simulation_config", config);
    h5::unlink_if_present(out, "particle_types");
    h5::hid ds(H5Dcreate2(out, "particle_types", ttype, tspace, H5P_DEFAULT, H5P_DEFAULT, H5P_DEFAULT));
    h5::check(ds >= 0, "cannot create metadata/particle_types");
    if (nt > 0) h5::check(H5Dwrite(ds, ttype, H5S_ALL, H5S_ALL, H5P_DEFAULT, tdata.data()) >= 0, "cannot write metadata/particle_types");
    cli::put(out, "chromosome_ranges", ranges.data(), {rows, 2}, nullptr);
    h5::write_fixed_string_list(out, "chromosome_names", names);
}

inline void run_distance(options const &o)
{
    device dev;
    open(dev);
    h5::hid file(cli::open_output(o.outfile));
    cli::stopwatch sw;
    copy_metadata(o.trajfiles[0], file);
    history cur = load_history(o.trajfiles[0]);
    sw.read += sw.lap();
    cli::filters f;
    f.scaleoffset_kind = H5Z_SO_FLOAT_DSCALE;
    f.scaleoffset_factor = 3;
    for (std::size_t k = 0; k < o.trajfiles.size(); k++) {
        // the next file is read while the device works; HDF5 is called from one thread at a time, so the write waits for it
        std::future<history> next;
        if (k + 1 < o.trajfiles.size()) next = std::async(std::launch::async, load_history, o.trajfiles[k + 1]);
        std::vector<float> dist((std::size_t)cur.frames * cur.beads);
        cli::check(gd_lamina_distances(dev.h, cur.xyz.data(), 0, cur.frames, cur.beads, cur.semiaxes.data(), dist.data(), 0));
        sw.compute += sw.lap();
        history following = next.valid() ? next.get() : history{};      // (a std::async future joins its thread when it is dropped)
        sw.read += sw.lap();
        cli::put(file, "/distance/" + cli::sample_name(o.trajfiles[k]), dist.data(), {cur.frames, cur.beads}, &f);
        sw.write += sw.lap();
        cur = std::move(following);
    }
    sw.report("gd_analyze_lamina distance");
}

inline herr_t collect_name(hid_t, const char *name, const H5L_info_t *, void *data)
{
    static_cast<std::vector<std::string> *>(data)->push_back(name);
    return 0;
}

inline void run_contact(options const &o)
{
    device dev;
    open(dev);
    h5::hid file(cli::open_output(o.outfile));
    cli::stopwatch sw;
    h5::hid group(H5Gopen2(file, "/distance", H5P_DEFAULT));
    h5::check(group >= 0, o.outfile + ": no /distance");
    std::vector<std::string> keys;      // in name order, as h5py iterates a group
    h5::check(H5Literate(group, H5_INDEX_NAME, H5_ITER_INC, nullptr, collect_name, &keys) >= 0, "cannot list /distance");
    h5::check(!keys.empty(), o.outfile + ": /distance is empty");
    h5::hid boolean(H5Tenum_create(H5T_STD_I8LE));      // h5py's bool
    std::int8_t const no = 0, yes = 1;
    H5Tenum_insert(boolean, "FALSE", &no);
    H5Tenum_insert(boolean, "TRUE", &yes);
    cli::filters const f;
    hsize_t dims[2] = {0, 0};
    for (auto const &key : keys) {
        h5::hid ds(H5Dopen2(group, key.c_str(), H5P_DEFAULT));
        h5::check(ds >= 0, "cannot open /distance/" + key);
        h5::hid space(H5Dget_space(ds));
        h5::check(H5Sget_simple_extent_ndims(space) == 2, "/distance/" + key + ": expected a 2-d dataset");
        H5Sget_simple_extent_dims(space, dims, nullptr);
        h5::check(dims[0] <= UINT32_MAX && dims[1] <= UINT32_MAX, "/distance/" + key + ": too large");
        std::vector<float> dist(dims[0] * dims[1]);
        if (!dist.empty()) h5::check(H5Dread(ds, H5T_NATIVE_FLOAT, H5S_ALL, H5S_ALL, H5P_DEFAULT, dist.data()) >= 0, "cannot read /distance/" + key);
        sw.read += sw.lap();
        std::vector<uint8_t> contacts(dist.size());
        cli::check(gd_lamina_contacts(dev.h, dist.data(), (uint32_t)dims[0], (uint32_t)dims[1], o.contact_distance, contacts.data()));
        sw.compute += sw.lap();
        cli::put_dataset(file, "/contact/" + o.name + "/" + key, contacts.data(), {dims[0], dims[1]}, 1, boolean, boolean, &f);
        sw.write += sw.lap();
    }
    std::vector<float> average(dims[0] * dims[1]);
    cli::check(gd_lamina_average(dev.h, average.data()));
    sw.compute += sw.lap();
    cli::put(file, "/average_contact/" + o.name, average.data(), {dims[0], dims[1]}, &f);
    sw.write += sw.lap();
    sw.report("gd_analyze_lamina contact");
}

// status 0, 1 (error: <what>) or 2 (usage)
inline int main(int argc, char **argv)
{
    options o;
    return cli::run(usage(), "gd_analyze_lamina", "error:", [&](std::string &err) { return parse(argc, argv, o, err); },
                    [&o] { return o.dry_run && (print_plan(o), true); }, [&o] {
        if (o.command == "distance") run_distance(o);
        else run_contact(o);
        return 0;
    });
}

}  // namespace lamina
}  // namespace gd
