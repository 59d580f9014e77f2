// gd_cli_util.hpp -- what the analysis programs share whatever they analyse: the option scanner (gd_cli_args.hpp), Python's
// repr of a float, the sample name of a trajectory file, the HDF5 datasets and groups of an output file as h5py writes them
// (put_dataset with its filters, put typed on the data), the error check of a libgdyn call, the read / compute / write
// stopwatch, the owner of a device handle (handle) and the one shape of a main (run).
#pragma once
#include <hdf5.h>

#include <algorithm>
#include <cerrno>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/gdyn.h"
#include "gd_cli_args.hpp"
#include "gd_h5util.hpp"

namespace gd {
namespace cli {

// repr(float) of Python: the shortest round-trip digits, fixed notation for exponents in [-4, 16), else d.ddde+XX
inline std::string py_float(double v)
{
    if (std::isnan(v)) return "NaN";                       // json.dumps spellings
    if (std::isinf(v)) return v > 0 ? "Infinity" : "-Infinity";
    char buf[64];
    auto res = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string s(buf, res.ptr);
    std::string sign;
    if (s[0] == '-') { sign = "-"; s = s.substr(1); }
    auto const e = s.find('e');
    int const exp10 = std::atoi(s.c_str() + e + 1);
    std::string digits;
    for (std::size_t k = 0; k < e; k++) if (s[k] != '.') digits += s[k];
    if (exp10 >= -4 && exp10 < 16) {
        std::string out;
        if (exp10 < 0) out = "0." + std::string((std::size_t)(-exp10 - 1), '0') + digits;
        else if ((int)digits.size() <= exp10 + 1) out = digits + std::string((std::size_t)(exp10 + 1 - (int)digits.size()), '0') + ".0";
        else out = digits.substr(0, (std::size_t)exp10 + 1) + "." + digits.substr((std::size_t)exp10 + 1);
        return sign + out;
    }
    std::string mant = digits.substr(0, 1);
    if (digits.size() > 1) mant += "." + digits.substr(1);
    char ex[16];
    std::snprintf(ex, sizeof ex, "e%c%02d", exp10 < 0 ? '-' : '+', std::abs(exp10));
    return sign + mant + ex;
}

inline std::string sample_name(std::string const &path)      // os.path.splitext(os.path.basename(path))[0]
{
    std::string b = path.substr(path.rfind('/') == std::string::npos ? 0 : path.rfind('/') + 1);
    auto dot = b.rfind('.');
    if (dot != std::string::npos && dot != 0 && b.find_first_not_of('.') < dot) b = b.substr(0, dot);
    return b;
}

struct filters {
    bool shuffle = true;
    int deflate = 1;
    int scaleoffset_kind = -1;          // H5Z_SO_FLOAT_DSCALE / H5Z_SO_INT, or -1: none
    int scaleoffset_factor = 0;
};

// put_dataset: an n-d array, replaced if present; chunks of at most 1 MiB along the leading axes (h5py chunks any filtered dataset)
inline void put_dataset(hid_t loc, std::string const &path, void const *data, std::vector<hsize_t> const &dims, std::size_t elem,
                        hid_t mem_type, hid_t file_type, filters const *f)
{
    h5::unlink_if_present(loc, path);
    h5::hid space(H5Screate_simple((int)dims.size(), dims.data(), nullptr)), props(H5Pcreate(H5P_DATASET_CREATE)),
        lcpl(H5Pcreate(H5P_LINK_CREATE));
    H5Pset_create_intermediate_group(lcpl, 1);
    hsize_t count = 1;
    for (auto d : dims) count *= d;
    if (f && count > 0) {
        std::vector<hsize_t> chunk(dims);
        for (std::size_t a = 0; a < chunk.size(); a++) {
            hsize_t bytes = elem;
            for (std::size_t b = 0; b < chunk.size(); b++) bytes *= chunk[b];
            if (bytes <= (1u << 20)) break;
            hsize_t rest = bytes / chunk[a];
            chunk[a] = std::max<hsize_t>(1, (1u << 20) / rest);
        }
        H5Pset_chunk(props, (int)chunk.size(), chunk.data());
        if (f->scaleoffset_kind >= 0) H5Pset_scaleoffset(props, (H5Z_SO_scale_type_t)f->scaleoffset_kind, f->scaleoffset_factor);
        if (f->shuffle) H5Pset_shuffle(props);
        if (f->deflate >= 0) H5Pset_deflate(props, (unsigned)f->deflate);
    }
    h5::hid ds(H5Dcreate2(loc, path.c_str(), file_type, space, lcpl, props, H5P_DEFAULT));
    h5::check(ds >= 0, "cannot create " + path);
    if (count) h5::check(H5Dwrite(ds, mem_type, H5S_ALL, H5S_ALL, H5P_DEFAULT, data) >= 0, "cannot write " + path);
}

// the HDF5 types of an element type: {in memory, in the file as h5py stores a numpy array of it}
template <typename T>
std::pair<hid_t, hid_t> h5_types()
{
    if constexpr (std::is_same_v<T, float>) return {H5T_NATIVE_FLOAT, H5T_IEEE_F32LE};
    else if constexpr (std::is_same_v<T, double>) return {H5T_NATIVE_DOUBLE, H5T_IEEE_F64LE};
    else if constexpr (std::is_same_v<T, int32_t>) return {H5T_NATIVE_INT32, H5T_STD_I32LE};
    else if constexpr (std::is_same_v<T, uint32_t>) return {H5T_NATIVE_UINT32, H5T_STD_U32LE};
    else if constexpr (std::is_same_v<T, int64_t>) return {H5T_NATIVE_INT64, H5T_STD_I64LE};
    else {
        static_assert(std::is_same_v<T, uint64_t>, "no HDF5 type for this element type: use put_dataset");
        return {H5T_NATIVE_UINT64, H5T_STD_U64LE};
    }
}

// put: put_dataset of an array whose file type is its element type's own
template <typename T>
void put(hid_t loc, std::string const &path, T const *data, std::vector<hsize_t> const &dims, filters const *f)
{
    put_dataset(loc, path, data, dims, sizeof(T), h5_types<T>().first, h5_types<T>().second, f);
}

inline hid_t open_output(std::string const &path)      // h5py.File(path, "a")
{
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    hid_t f = std::ifstream(path).good() ? H5Fopen(path.c_str(), H5F_ACC_RDWR, H5P_DEFAULT)
                                                            : H5Fcreate(path.c_str(), H5F_ACC_EXCL, H5P_DEFAULT, H5P_DEFAULT);
    h5::check(f >= 0, "cannot open " + path);
    return f;
}

inline hid_t require_group(hid_t file, std::string const &path)      // put_group
{
    if (H5Lexists(file, path.c_str(), H5P_DEFAULT) > 0) return H5Gopen2(file, path.c_str(), H5P_DEFAULT);
    h5::hid lcpl(H5Pcreate(H5P_LINK_CREATE));
    H5Pset_create_intermediate_group(lcpl, 1);
    hid_t g = H5Gcreate2(file, path.c_str(), lcpl, H5P_DEFAULT, H5P_DEFAULT);
    h5::check(g >= 0, "cannot create group " + path);
    return g;
}

// every failure of the library ends the program with its message
inline void check(int rc)
{
    if (rc != GD_OK) throw std::runtime_error(std::string("gdyn: ") + gd_last_error());
}

struct stopwatch {
    double read = 0, compute = 0, write = 0;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    double lap()
    {
        auto const now = std::chrono::steady_clock::now();
        double const s = std::chrono::duration<double>(now - t).count();
        t = now;
        return s;
    }
    void report(char const *prog) const { std::fprintf(stderr, "%s: read %.3f s, compute %.3f s, write %.3f s\n", prog, read, compute, write); }
};

// one handle of a device module, owned.  open(create) makes it on first use, where create(&h) is the module's create call (a
// program that opens it after its first read reports a missing input as such); every failure of the library ends the program
template <typename H, auto Destroy>
struct handle {
    H *h = nullptr;
    double startup = 0;      // seconds the create call took (the HIP runtime starts there), inside whichever lap the caller opens it in
    handle() = default;
    handle(handle const &) = delete;
    handle &operator=(handle const &) = delete;
    ~handle() { Destroy(h); }
    template <typename Create>
    void open(Create &&create)
    {
        if (h) return;
        auto const t = std::chrono::steady_clock::now();
        check(create(&h));
        startup = std::chrono::duration<double>(std::chrono::steady_clock::now() - t).count();
    }
    void report(char const *prog) const { std::fprintf(stderr, "%s: device start-up %.3f s\n", prog, startup); }
};

// the one main shape: a message of parse(err) after the usage text is status 2; plan() serves a --dry-run that needs no file and
// says whether it did; then body() under the catch, where an exception is status 1 after `error_prefix`.  A program whose
// --dry-run reads its inputs passes no_plan and serves it at the head of body
inline bool no_plan() { return false; }

template <typename Parse, typename Plan, typename Body>
int run(std::string const &usage, char const *prog, char const *error_prefix, Parse &&parse, Plan &&plan, Body &&body)
{
    std::string err;
    if (parse(err)) {
        std::fprintf(stderr, "%s%s: error: %s\n", usage.c_str(), prog, err.c_str());
        return 2;
    }
    if (plan()) return 0;
    try {
        H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
        return body();
    } catch (std::exception const &e) {
        std::fprintf(stderr, "%s %s\n", error_prefix, e.what());
        return 1;
    }
}

}  // namespace cli
}  // namespace gd
