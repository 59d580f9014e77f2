// gdyn_history.hip -- gd::History (gdyn_history.hpp): the upload or the strided device copy of a history, and
//   k_history_first_bad  the lowest index of a non-finite coordinate (integer atomicMin, reached by no lane of a finite history)
#include "gdyn_history.hpp"

#include <numeric>

using namespace gd;

namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 8192;        // of the scan; longer histories are walked with a grid stride
constexpr unsigned long long kNoBadIndex = ~0ull;

template <typename T>
__global__ void __launch_bounds__(kBlock) k_history_first_bad(const T *__restrict__ x, size_t n, unsigned long long *first_bad)
{
    unsigned long long bad = kNoBadIndex;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kBlock)
        if (!isfinite(x[i])) bad = min(bad, (unsigned long long)i);
    if (bad != kNoBadIndex) atomicMin(first_bad, bad);
}

int check_shape(const char *who, uint32_t frames, uint32_t n_beads)
{
    if (frames == 0 || n_beads == 0) return fail(GD_EINVAL, "%s: empty history (%u frames of %u beads)", who, frames, n_beads);
    if (n_beads > (1u << 28)) return fail(GD_EINVAL, "%s: %u beads exceed 2^28", who, n_beads);
    return GD_OK;
}

}  // namespace

namespace gd {

// the history is on the device: the non-finite check, then the handle holds it (or none)
int History::finish(const char *who, hipStream_t stream, unsigned frames, unsigned n_beads, bool f64, const Rebind &rebind)
{
    size_t const n = (size_t)frames * n_beads * 3;
    HIPCHK(first_bad.ensure(1));
    HIPCHK(hipMemsetAsync(first_bad.p, 0xff, sizeof(unsigned long long), stream));
    unsigned const blocks = (unsigned)std::min<size_t>((n + kBlock - 1) / kBlock, kMaxBlocks);
    if (f64) hipLaunchKernelGGL(k_history_first_bad<double>, dim3(blocks), dim3(kBlock), 0, stream, xd.p, n, first_bad.p);
    else hipLaunchKernelGGL(k_history_first_bad<float>, dim3(blocks), dim3(kBlock), 0, stream, xf.p, n, first_bad.p);
    HIPCHK(hipGetLastError());
    unsigned long long bad = kNoBadIndex;
    HIPCHK(hipMemcpyAsync(&bad, first_bad.p, sizeof bad, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    if (bad != kNoBadIndex) return fail(GD_EINVAL, "%s: non-finite coordinate at %llu", who, bad);
    GDCHK(rebind(n_beads));
    F = frames;
    N = n_beads;
    is_f64 = f64;
    return GD_OK;
}

int History::set_host(const char *who, int device, hipStream_t stream, const void *xyz, uint32_t frames, uint32_t n_beads, bool f64, const Rebind &rebind)
{
    if (!xyz) return fail(GD_EINVAL, "%s: NULL argument", who);
    GDCHK(check_shape(who, frames, n_beads));
    HIPCHK(hipSetDevice(device));
    size_t const n = (size_t)frames * n_beads * 3;
    F = 0;      // the buffer is about to be overwritten
    if (f64) HIPCHK(xd.upload(static_cast<const double *>(xyz), n));
    else HIPCHK(xf.upload(static_cast<const float *>(xyz), n));
    return finish(who, stream, frames, n_beads, f64, rebind);
}

int History::set_live(const char *who, int device, hipStream_t stream, gd_live_history *history, uint32_t replica, const Rebind &rebind)
{
    if (!history) return fail(GD_EINVAL, "%s: NULL handle", who);
    gd_live_history_shape const v = gd_live_history_shape_of(history);
    uint32_t slot = 0;
    GDCHK(gd_live_history_slot(history, who, replica, &slot));
    if (v.device != device) return fail(GD_EINVAL, "%s: the recorder is on device %d, the analysis handle on device %d", who, v.device, device);
    if (!v.frames) return fail(GD_ESTATE, "%s: no frame recorded", who);
    GDCHK(check_shape(who, v.frames, v.N));
    HIPCHK(hipSetDevice(device));
    size_t const M = (size_t)v.N * 3;
    F = 0;
    HIPCHK(xf.ensure((size_t)v.frames * M));
    for (uint32_t f0 = 0; f0 < v.frames; f0 += v.frames_per_block) {      // one strided copy per block of the recorder
        uint32_t const nf = std::min(v.frames_per_block, v.frames - f0);
        HIPCHK(hipMemcpy2DAsync(xf.p + (size_t)f0 * M, M * sizeof(float), gd_live_history_frame(history, f0, slot), v.frame_stride * sizeof(float),
                                M * sizeof(float), nf, hipMemcpyDeviceToDevice, stream));
    }
    return finish(who, stream, v.frames, v.N, false, rebind);
}

int check_ranges(const char *who, const char *noun, bool empty_allowed, const uint32_t *r, unsigned count, unsigned N)
{
    for (unsigned c = 0; c < count; c++) {
        if (empty_allowed ? r[2 * c] > r[2 * c + 1] : r[2 * c] >= r[2 * c + 1])
            return fail(GD_EINVAL, "%s: %s %u is %s: [%u, %u)", who, noun, c, empty_allowed ? "reversed" : "empty or reversed", r[2 * c], r[2 * c + 1]);
        if (r[2 * c + 1] > N) return fail(GD_EINVAL, "%s: %s %u ends at %u, beyond the %u beads", who, noun, c, r[2 * c + 1], N);
        if (c && r[2 * c] < r[2 * c - 1])
            return fail(GD_EINVAL, "%s: %s %u starts at %u, before %s %u ends (%u)", who, noun, c, r[2 * c], noun, c - 1, r[2 * c - 1]);
    }
    return GD_OK;
}

int check_labels(const char *who, const char *noun, const int32_t *label, unsigned N, unsigned K)
{
    if (!label) return K > 1 ? fail(GD_EINVAL, "%s: %u %ss without a %s array", who, K, noun, noun) : GD_OK;
    for (unsigned i = 0; i < N; i++)
        if (label[i] < -1 || label[i] >= (int64_t)K) return fail(GD_EINVAL, "%s: %s[%u] = %d is not in [-1, %u)", who, noun, i, label[i], K);
    return GD_OK;
}

int LabelSelection::select_all(unsigned N)
{
    std::vector<unsigned> all(N);
    std::iota(all.begin(), all.end(), 0u);
    dbuf<unsigned> dev;
    HIPCHK(dev.upload(all.data(), N));
    sel = std::move(dev);
    n_sel = N;
    K = 1;
    have_labels = false;
    members.assign(1, N);
    return GD_OK;
}

int LabelSelection::set(const char *who, int device, const int32_t *label, uint32_t n_labels, unsigned max_labels, unsigned N)
{
    if (!label) {
        GDCHK(check_labels(who, "label", nullptr, N, n_labels));
        HIPCHK(hipSetDevice(device));
        return select_all(N);
    }
    if (n_labels == 0 || n_labels > max_labels) return fail(GD_EINVAL, "%s: %u labels (1 to %u)", who, n_labels, max_labels);
    GDCHK(check_labels(who, "label", label, N, n_labels));
    std::vector<unsigned> chosen;
    std::vector<uint64_t> count(n_labels, 0);
    for (unsigned i = 0; i < N; i++)
        if (label[i] >= 0) {
            chosen.push_back(i);
            count[label[i]]++;
        }
    HIPCHK(hipSetDevice(device));
    dbuf<unsigned> s;
    dbuf<int> dev;
    HIPCHK(s.upload(chosen.data(), chosen.size()));
    HIPCHK(dev.upload(label, N));
    sel = std::move(s);
    label_dev = std::move(dev);
    n_sel = (unsigned)chosen.size();
    K = n_labels;
    have_labels = true;
    members = std::move(count);
    return GD_OK;
}

int BeadRanges::install(std::vector<uint32_t> ranges, bool have_now)
{
    dbuf<uint32_t> d;
    HIPCHK(d.upload(ranges.data(), ranges.size()));
    dev = std::move(d);
    host = std::move(ranges);
    have = have_now;
    return GD_OK;
}

int BeadRanges::every_bead(unsigned N)
{
    std::vector<uint32_t> r(2 * (size_t)N);
    for (unsigned i = 0; i < N; i++) {
        r[2 * (size_t)i] = i;
        r[2 * (size_t)i + 1] = i + 1;
    }
    return install(std::move(r), false);
}

int BeadRanges::set(const char *who, const char *noun, int device, const uint32_t *ranges, uint32_t n, unsigned limit_bits, unsigned N)
{
    if (n > (1u << limit_bits)) return fail(GD_EINVAL, "%s: %u %ss exceed 2^%u", who, n, noun, limit_bits);
    HIPCHK(hipSetDevice(device));
    if (!n) return every_bead(N);
    GDCHK(check_ranges(who, noun, false, ranges, n, N));
    return install(std::vector<uint32_t>(ranges, ranges + 2 * (size_t)n), true);
}

}  // namespace gd
