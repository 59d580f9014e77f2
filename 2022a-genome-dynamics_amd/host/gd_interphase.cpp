// gd_interphase -- the 100 kb whole-genome relaxation + interphase driver on libgdyn.
//
// Mirrors the reference program `simulation_interphase <trajectory.h5>`
// (5-sim-genome/src/simulation_interphase/: main.cc:15-27, simulation_driver.cc:15-58,
// simulation_driver_particles.cc:8-36, simulation_driver_forcefield.cc:8-235,
// simultion_driver_relaxation.cc:8-46, simulation_driver_interphase.cc:8-80): same input/output file, same
// config keys, same phases, same log lines, same snapshot cadence.  The micromd calls are replaced by the
// C-ABI of include/gdyn.h; the per-step callback state (time, scales, wall ODE) advances on the device and the
// host only intervenes at logging / sampling / contact-map steps.
//
// Differences from the reference, by construction: fp32 device arithmetic and a Philox noise stream (micromd's
// generator is not reproducible); `spacestep` must be 0; the softwell droplet force
// (nucleolus_droplet_energy != 0) uses a documented choice of micromd's potential form (include/gdyn.h).
//
// --ensemble-matrix RATE OUTPUT (not in the reference): the genome-wide contact matrix of the run's replicas, summed on the
// device from the contact tables each time they are dumped (gd_live_contacts, include/gdyn_live.h) and written at the end
// exactly as `gd_gw_contact_matrix --rebin-rate RATE -o OUTPUT <the same files>` writes it from the stored maps afterwards.
//
// Files that differ in /metadata/ab_factors alone -- a genome model and its randomised controls (gd_randomize.py), other annotations of
// one genome -- batch as well: replica r takes its (a, b) factors from file r (gd_ensemble_set_ab, include/gdyn_ensemble.h).  The
// files with equal factors form a model, numbered by first appearance in file order and named on stderr, `[model k] file ...`.
// --ensemble-matrix then pools per model: OUTPUT must contain {model}, which the model's number replaces, and model k's file holds
// what `gd_gw_contact_matrix --rebin-rate RATE -o ... <the files of model k>` writes.  (A batch of one model: one matrix as before,
// {model} -- if OUTPUT has it -- replaced by 0.)  The flow outputs are per replica and need nothing for this.
//
// --particle-flow OUTPUT, --grid-flow OUTPUT (not in the reference): the flow fields of the run's replicas.  Every frame stored under
// snapshots/interphase is also recorded on the device (gd_live_history, include/gdyn_live.h), and at the end one gd_flow handle
// works through the replicas in file order and writes exactly what `gd_particle_flow OUTPUT <flow options> <the same files>` and
// `gd_grid_flow OUTPUT ...` write from the stored frames afterwards.  The flow options are theirs (gd_flow_cli.hpp) and shared.
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <ctime>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_ensemble.h"
#include "../../include/gdyn_live.h"
// This program is also linked against libraries that implement gdyn.h alone (the fp64 oracle of the tests).  What
// --ensemble-matrix and the flow options call is referenced weakly, and the options are refused where the symbols are absent;
// so are the per-replica A/B tables, without which a batch of differing models is refused.
#pragma weak gd_ensemble_set_ab
#pragma weak gd_ensemble_classes
#pragma weak gd_cmap_create
#pragma weak gd_cmap_destroy
#pragma weak gd_cmap_add_binned
#pragma weak gd_cmap_target_size
#pragma weak gd_cmap_fetch
#pragma weak gd_live_contacts
#pragma weak gd_flow_create
#pragma weak gd_flow_destroy
#pragma weak gd_flow_velocities
#pragma weak gd_flow_particle
#pragma weak gd_flow_grid
#pragma weak gd_live_history_create
#pragma weak gd_live_history_destroy
#pragma weak gd_live_history_record
#pragma weak gd_live_history_frames
#pragma weak gd_live_history_fetch
#pragma weak gd_live_flow_set_history
#include "gd_async_io.hpp"
#include "gd_cmap_cli.hpp"
#include "gd_flow_cli.hpp"
#include "gd_config.hpp"
#include "gd_genome_model.hpp"
#include "gd_store.hpp"

namespace {

using gd::chk;

// --timing: where the wall time of a run goes (stepping thread and writer thread), one line on stderr at the end
class timing_table {
public:
    struct scope {
        timing_table &t; char const *name; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        ~scope() { t.add(name, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count()); }
    };
    void add(char const *name, double seconds) { std::lock_guard<std::mutex> lk(_m); _t[name] += seconds; }
    void note(std::string const &line) { std::lock_guard<std::mutex> lk(_m); _notes.push_back(line); }
    void print() const
    {
        for (auto const &n : _notes) std::clog << "[timing] " << n << '\n';
        std::clog << "[timing]";
        for (auto const &kv : _t) std::clog << ' ' << kv.first << ' ' << std::fixed << std::setprecision(3) << kv.second;
        std::clog << '\n';
    }
private:
    std::mutex _m;
    std::map<std::string, double> _t;
    std::vector<std::string> _notes;
};
timing_table g_timing;
#define GD_CONCAT2(a, b) a##b
#define GD_CONCAT(a, b) GD_CONCAT2(a, b)      // (two levels: __LINE__ expands before the paste)
#define TIMED(name) timing_table::scope GD_CONCAT(timed_scope_, __LINE__){g_timing, name}

// Time-integrated contact maps (simulation_interphase/contact_map.cc:26-91) live on the device, one per replica (gd_contacts_*):
// an update is one pair search over all replicas plus one insert launch, and only a dump moves rows to the host.
std::vector<std::array<std::uint32_t, 3>> fetch_contacts(gd_system *sys, uint32_t replica)
{
    uint64_t n = 0;
    chk(gd_contacts_fetch(sys, replica, nullptr, 0, &n));
    std::vector<std::array<std::uint32_t, 3>> rows(n);
    if (n) chk(gd_contacts_fetch(sys, replica, rows.data()->data(), n, &n));
    return rows;
}

// --ensemble-matrix: one binned target over the chromosome ranges of the first file (gd_gw_contact_matrix's rebin rule), fed
// from the device-resident contact tables of all replicas
struct ensemble_matrix {
    std::string output;
    gd::cmap::trajectory head;
    gd::cmap::rebinning rb;
    gd::cmap::device dev;
    int32_t target = -1;

    static bool available() { return gd_cmap_create && gd_cmap_destroy && gd_cmap_add_binned && gd_cmap_target_size && gd_cmap_fetch && gd_live_contacts; }
    ensemble_matrix(std::string const &first_file, long rate, std::string const &out, int device)
        : output(out), head(gd::cmap::load_ranges(first_file)), rb(gd::cmap::rebin(head, rate))
    {
        gd::cmap::open(dev, device);
        gd::cli::check(gd_cmap_add_binned(dev.h, rb.map.data(), (uint32_t)rb.map.size(), rb.n_bins, &target));
    }
    void add(gd_system *sys, uint32_t replica) { gd::cli::check(gd_live_contacts(sys, replica, dev.h)); }
    void write() { gd::cmap::write_gw_matrix(output, head, rb, gd::cmap::fetch(dev, target)); }
};

// The models of a batch: files whose /metadata/ab_factors are equal, numbered by first appearance in file order
struct model_classes {
    std::vector<uint32_t> of;      // by file
    uint32_t n = 0;
    std::vector<std::string> files_of(std::vector<std::string> const &files, uint32_t k) const
    {
        std::vector<std::string> v;
        for (std::size_t r = 0; r < files.size(); r++) if (of[r] == k) v.push_back(files[r]);
        return v;
    }
};

// the factors of a prepared file, read before the stores open the files for writing
std::vector<double> load_ab_factors(std::string const &path)
{
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    hid_t const file = H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
    gd::h5::check(file >= 0, "cannot open " + path);
    std::vector<double> ab;
    try {
        gd::h5::hid meta(H5Gopen2(file, "/metadata", H5P_DEFAULT));
        gd::h5::check(meta >= 0, path + ": no /metadata");
        ab = gd::h5::read_array<double>(meta, "ab_factors", 2, H5T_NATIVE_DOUBLE);
    } catch (...) {
        H5Fclose(file);
        throw;
    }
    H5Fclose(file);
    return ab;
}

model_classes classify_models(std::vector<std::string> const &files)
{
    model_classes m;
    std::vector<std::vector<double>> first;      // the factors of every model's first file
    for (auto const &f : files) {
        auto ab = load_ab_factors(f);
        std::size_t k = 0;
        while (k < first.size() && first[k] != ab) k++;
        if (k == first.size()) first.push_back(std::move(ab));
        m.of.push_back((uint32_t)k);
    }
    m.n = (uint32_t)first.size();
    return m;
}

// --ensemble-matrix of a run: one matrix over all replicas, or one per model, each fed from the replicas of its model
struct ensemble_matrices {
    std::vector<std::unique_ptr<ensemble_matrix>> of_model;
    std::vector<uint32_t> model_of;      // by replica

    static std::string output_name(std::string name, uint32_t model)
    {
        std::string const key = "{model}";
        for (std::size_t at; (at = name.find(key)) != std::string::npos;) name.replace(at, key.size(), std::to_string(model));
        return name;
    }
    ensemble_matrices(std::vector<std::string> const &files, model_classes const &models, long rate, std::string const &out, int device)
        : model_of(models.of)
    {
        for (uint32_t k = 0; k < models.n; k++)
            of_model.push_back(std::make_unique<ensemble_matrix>(models.files_of(files, k).front(), rate, output_name(out, k), device));
    }
    void add(gd_system *sys)
    {
        if (of_model.size() == 1) { of_model[0]->add(sys, GD_ALL_REPLICAS); return; }
        for (std::size_t r = 0; r < model_of.size(); r++) of_model[model_of[r]]->add(sys, (uint32_t)r);
    }
    void write() { for (auto &m : of_model) m->write(); }
};

// --particle-flow / --grid-flow: the interphase frames recorded on the device as they are stored, and the two analyses of them
struct flow_outputs {
    gd::flow::options particle, grid;      // outfile empty: not asked for.  Both hold the shared flow options
    gd_live_history *history = nullptr;
    uint32_t beads = 0;

    static bool available()
    {
        return gd_flow_create && gd_flow_destroy && gd_flow_velocities && gd_flow_particle && gd_flow_grid && gd_live_history_create &&
               gd_live_history_destroy && gd_live_history_record && gd_live_history_frames && gd_live_history_fetch && gd_live_flow_set_history;
    }
    ~flow_outputs() { if (history) gd_live_history_destroy(history); }
    // all replicas, automatic blocks; `frames` is what the run will store
    void open(gd_system *sys, std::size_t replicas, std::size_t frames, std::size_t n)
    {
        beads = (uint32_t)n;
        std::clog << "[flow] recording " << frames << " frames of " << replicas << " replicas of " << n << " beads on the device: "
                  << replicas * frames * n * 12 << " bytes\n";
        gd::cli::check(gd_live_history_create(sys, nullptr, 0, 0, &history));
    }
    void record(gd_system *sys) { gd::cli::check(gd_live_history_record(history, sys, /*quantize=*/1)); }
    uint32_t frames() const
    {
        uint32_t f = 0;
        gd::cli::check(gd_live_history_frames(history, &f));
        return f;
    }
    void write(std::vector<std::string> const &files, int ordinal)
    {
        using namespace gd::flow;
        uint32_t const F = frames(), N = beads;
        options const &o = particle.outfile.empty() ? grid : particle;      // (the velocity options are the same in both)
        bool const smooth = smoothed(o);
        gd::flow::device dev;
        gd::flow::open(dev, ordinal);
        std::unique_ptr<particle_writer> pw;
        std::unique_ptr<grid_writer> gw;
        std::unique_ptr<mesh> m;
        if (!particle.outfile.empty()) {
            std::string const config = config_json(particle, false);
            pw = std::make_unique<particle_writer>(particle.outfile, analysis_name(particle, config), config);
        }
        if (!grid.outfile.empty()) {
            std::string const config = config_json(grid, true);
            m = std::make_unique<mesh>(grid);
            gw = std::make_unique<grid_writer>(grid.outfile, analysis_name(grid, config), config, *m);
        }
        for (std::size_t r = 0; r < files.size(); r++) {
            std::string const sample = gd::cli::sample_name(files[r]);
            gd::cli::check(gd_live_flow_set_history(history, (uint32_t)r, dev.h));
            std::vector<double> pos(pw && smooth ? (std::size_t)F * N * 3 : 0);
            gd::cli::check(gd_flow_velocities(dev.h, smooth ? (uint32_t)o.smoothing : 0, (uint32_t)o.delay, pos.empty() ? nullptr : pos.data(), nullptr));
            if (pw) {
                std::vector<float> flows((std::size_t)F * N * 3), hist(smooth ? 0 : (std::size_t)F * N * 3);
                gd::cli::check(gd_flow_particle(dev.h, o.radius, flows.data()));
                if (!smooth) gd::cli::check(gd_live_history_fetch(history, (uint32_t)r, 0, F, hist.data()));
                pw->put(sample, F, N, hist.data(), smooth ? pos.data() : nullptr, flows.data());
            }
            if (gw) {
                std::vector<float> flows((std::size_t)F * m->G * 3);
                std::vector<int32_t> cov((std::size_t)F * m->G);
                gd::cli::check(gd_flow_grid(dev.h, o.radius, m->points.data(), (uint32_t)m->G, flows.data(), cov.data()));
                gw->put(sample, F, flows, cov, scaleoffset_factor(flows));
            }
        }
        if (pw) pw->finish();
        if (gw) gw->finish();
    }
};

// One driver = one libgdyn handle = R replicas = R trajectory files.  R = 1 is the reference program; R > 1 batches R runs
// of the reference's ensemble (one process per seed, each with its own prepared file: 5-sim-genome/scripts/run_simulation:8-25,
// read back as output-*.h5 by contact_map/contact_map.py:14-39) into one launch: replica r takes its initial structure, its
// seeds and its outputs from file r; every replica draws the noise stream its own one-replica run would draw
// (gd_run_desc.replica_seeds), so a batched trajectory equals the solo one up to fp32 summation order.
class simulation_driver {
public:
    simulation_driver(std::vector<std::unique_ptr<gd::trajectory_store>> &stores, int device, bool auto_skin = false, ensemble_matrices *ensemble = nullptr,
                      flow_outputs *flow = nullptr, model_classes const *models = nullptr)
        : _stores(stores), _R(stores.size()), _config(gd::parse_simulation_config(stores[0]->load_config_text())), _auto_skin(auto_skin),
          _ensemble(ensemble), _flow(flow), _models(models)
    {
        // compatibility defaults of older runs (simulation_driver.cc:20-29)
        auto set_default = [](double &var, double def) { if (var == 0) var = def; };
        set_default(_config.a_core_bond_spring, _config.chromatin_bond_spring);
        set_default(_config.a_core_bond_length, _config.chromatin_bond_length);
        set_default(_config.b_core_bond_spring, _config.chromatin_bond_spring);
        set_default(_config.b_core_bond_length, _config.chromatin_bond_length);
        for (std::size_t r = 0; r < _R; r++) {
            auto const cfg = gd::parse_simulation_config(_stores[r]->load_config_text());
            // one handle runs one force field and one schedule: every config entry except the seeds must agree
            if (r > 0 && !gd::same_model_config(_stores[r]->load_config_text(), _stores[0]->load_config_text()))
                throw std::runtime_error("batched trajectories must share one simulation config (seeds aside)");
            _random.emplace_back(cfg.interphase_seed);          // 1st draw: relaxation seed, 2nd: interphase seed
        }
        TIMED("setup");
        setup(device);
    }
    ~simulation_driver() { gd_destroy(_sys); }

    void run()
    {
        g_timing.note("packing pool of " + std::to_string(gd::usable_threads()) + " threads on " + std::to_string(gd::usable_cpus()) + " usable CPUs");
        run_relaxation(); report("relaxation"); run_simulation(); report("interphase");
        TIMED("writer_wait");
        _writer.drain();
    }
    // bead-steps of the whole run (all files of this process): what a farm's per-device rate is made of
    double bead_steps() const { return (double)_n * (double)_R * (double)(_config.relaxation_steps + _config.interphase_steps); }
    void report(char const *phase)      // (--timing) the list statistics of the handle at the end of a phase
    {
        g_timing.note(std::string(phase) + ": " + std::to_string(_energy_calls) + " energy evaluations so far, " + std::to_string(_energy_builds) +
                      " list builds inside them, slowest " + std::to_string(_energy_max) + " s");
        gd_context c;
        chk(gd_get_context(_sys, 0, &c));
        char line[256];
        std::snprintf(line, sizeof line, "%s: list path %u, %.1f entries per bead, radius %.4f, interval %u, %llu builds, %llu rollbacks, lists %.2f GB",
                      phase, c.list_path, (double)c.list_entries / (double)_n, c.list_radius, c.rebuild_interval,
                      (unsigned long long)c.rebuilds, (unsigned long long)c.rollbacks, (double)c.list_bytes / 1e9);
        g_timing.note(line);
    }

private:
    void setup(int device)
    {
        _sys = gd::build_genome_system(*_stores[0], _config, device, /*loop_bonds=*/true, /*mixed_chain_bonds=*/true, _n, (uint32_t)_R);
        auto const p0 = _stores[0]->load_particle_data();
        bool tables = false;
        for (std::size_t r = 1; r < _R; r++) {
            auto const pr = _stores[r]->load_particle_data();
            if (pr.size() != p0.size()) throw std::runtime_error("batched trajectories must hold the same model (bead count differs)");
            bool differ = false;
            for (std::size_t i = 0; !differ && i < p0.size(); i++) differ = pr[i].a != p0[i].a || pr[i].b != p0[i].b;
            if (differ) {      // the replica carries its own factors, where the library has per-replica tables
                if (!gd_ensemble_set_ab || !gd_ensemble_classes)
                    throw std::runtime_error("batched trajectories must hold the same model (A/B factors differ)");
                std::vector<double> a(pr.size()), b(pr.size());
                for (std::size_t i = 0; i < pr.size(); i++) { a[i] = pr[i].a; b[i] = pr[i].b; }
                chk(gd_ensemble_set_ab(_sys, (uint32_t)r, a.data(), b.data()));
                tables = true;
            }
            // the topology the handle is built from is file 0's: chains, nucleolar ranges and bonds must agree as well
            auto const c0 = _stores[0]->load_chromosomes(), cr = _stores[r]->load_chromosomes();
            bool same = c0.size() == cr.size();
            for (std::size_t i = 0; same && i < c0.size(); i++) same = c0[i].start == cr[i].start && c0[i].end == cr[i].end;
            auto const n0 = _stores[0]->load_nucleolus_ranges(), nr = _stores[r]->load_nucleolus_ranges();
            same = same && n0.size() == nr.size();
            for (std::size_t i = 0; same && i < n0.size(); i++) same = n0[i].begin == nr[i].begin && n0[i].end == nr[i].end;
            auto const b0 = _stores[0]->load_nucleolus_bonds(), br = _stores[r]->load_nucleolus_bonds();
            same = same && b0.size() == br.size();
            for (std::size_t i = 0; same && i < b0.size(); i++) same = b0[i].nor_index == br[i].nor_index && b0[i].nuc_index == br[i].nuc_index;
            if (!same) throw std::runtime_error("batched trajectories must hold the same model (chromosome / nucleolus tables differ)");
        }
        if (tables) {      // the models as the library sees them are those the command line was checked against
            std::vector<uint32_t> of(_R);
            uint32_t n = 0;
            chk(gd_ensemble_classes(_sys, of.data(), &n));
            if (_models && (n != _models->n || of != _models->of)) throw std::runtime_error("the models of the batch changed between the check of the command line and the set-up");
        }
        // setup_context (simulation_driver.cc:43-51)
        gd::context c{};
        c.wall_semiaxes[0] = _config.wall_init_semiaxes.x; c.wall_semiaxes[1] = _config.wall_init_semiaxes.y;
        c.wall_semiaxes[2] = _config.wall_init_semiaxes.z;
        c.bead_scale = _config.bead_scale_init; c.bond_scale = _config.bond_scale_init;
        _context.assign(_R, c);
        {   // the list width follows the structure (a freshly refined genome is a dense globule that decondenses over the run): by
            // the library's rules on the state -- tile class, rows sized per wave -- so that a seed gives one trajectory, as in
            // the reference (scripts/run_simulation:8-25); --auto-skin selects it from measured chunk times instead
            gd_tuning tune{};
            tune.adapt_interval = 1; tune.auto_skin = _auto_skin ? 1 : 0;
            chk(gd_set_tuning(_sys, &tune));
        }
        _buffer.resize(3 * _n * _R);
        _energy.resize(_R);
        if (_flow) _flow->open(_sys, _R, (std::size_t)(_config.interphase_steps / _config.interphase_sampling_interval) + 1, _n);
    }

    std::vector<double> semiaxes() const
    {
        std::vector<double> v(3 * _R);
        for (std::size_t r = 0; r < _R; r++) std::copy(_context[r].wall_semiaxes, _context[r].wall_semiaxes + 3, v.begin() + 3 * r);
        return v;
    }

    void print_progress(char const *phase, long step)
    {
        std::time_t const now = std::time(nullptr);
        for (std::size_t r = 0; r < _R; r++) {
            auto const &c = _context[r];
            double const radius = std::cbrt(c.wall_semiaxes[0] * c.wall_semiaxes[1] * c.wall_semiaxes[2]);
            std::clog << "[" << phase;
            if (_R > 1) std::clog << ":" << r;
            std::clog << "] " << std::put_time(std::localtime(&now), "%F %T") << '\t' << step << '\t'
                      << "t: " << c.time << '\t' << "R: " << radius << '\t' << "E: " << c.mean_energy << '\n';
        }
    }

    void mean_energy()
    {
        TIMED("energy");
        gd_context before, after;
        chk(gd_get_context(_sys, 0, &before));
        auto const t0 = std::chrono::steady_clock::now();
        chk(gd_compute_energy(_sys, GD_TERM_ALL, _energy.data()));
        double const dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        chk(gd_get_context(_sys, 0, &after));
        _energy_calls++; _energy_builds += after.rebuilds - before.rebuilds; _energy_max = std::max(_energy_max, dt);
        for (std::size_t r = 0; r < _R; r++) _context[r].mean_energy = _energy[r] / (double)_n;
    }

    // Output leaves the stepping thread as a job (gd_async_io.hpp): the chunks of all R files are packed on the pool's threads, the
    // HDF5 calls follow on the writer thread, the device goes on stepping meanwhile.
    void save_snapshot(long step)
    {
        std::shared_ptr<std::vector<float>> xyz;
        {
            TIMED("snapshot_download");
            chk(gd_get_positions_f32(_sys, _buffer.data(), /*quantize=*/1));      // 16 fractional bits, rounded on the device
            xyz = std::make_shared<std::vector<float>>(_buffer);
        }
        if (_flow && _interphase) {      // the same frame, kept on the device
            TIMED("flow_record");
            _flow->record(_sys);
        }
        auto ctx = std::make_shared<std::vector<gd::context>>(_context);
        TIMED("writer_wait");
        _writer.submit([this, step, xyz, ctx] {
            std::vector<gd::h5::packed_array> packed(_R, gd::h5::plan_packed(_n, 3, sizeof(float)));
            std::size_t const per = packed[0].chunk_count();
            {
                TIMED("w:pack");
                _pool.parallel_for(_R * per, [&](std::size_t t) { gd::h5::pack_chunk(packed[t / per], t % per, xyz->data() + 3 * _n * (t / per)); });
            }
            TIMED("w:hdf5");
            for (std::size_t r = 0; r < _R; r++) {
                _stores[r]->save_positions_packed(step, packed[r]);
                _stores[r]->save_context(step, (*ctx)[r]);
            }
        });
    }

    void save_contacts(long step)
    {
        auto rows = std::make_shared<std::vector<std::vector<std::array<std::uint32_t, 3>>>>(_R);
        if (_ensemble) {      // the maps about to be dumped and cleared, summed where they lie
            TIMED("ensemble_matrix");
            _ensemble->add(_sys);
        }
        {
            TIMED("contacts_fetch");
            for (std::size_t r = 0; r < _R; r++) (*rows)[r] = fetch_contacts(_sys, (uint32_t)r);
            chk(gd_contacts_clear(_sys, GD_ALL_REPLICAS));
        }
        TIMED("writer_wait");
        _writer.submit([this, step, rows] {
            std::vector<gd::h5::packed_array> packed(_R);
            std::vector<std::pair<std::size_t, std::size_t>> tasks;
            for (std::size_t r = 0; r < _R; r++) {
                packed[r] = gd::h5::plan_packed((*rows)[r].size(), 3, sizeof(std::uint32_t));
                for (std::size_t c = 0; c < packed[r].chunk_count(); c++) tasks.push_back({r, c});
            }
            {
                TIMED("w:pack");
                _pool.parallel_for(tasks.size(), [&](std::size_t t) { gd::h5::pack_chunk(packed[tasks[t].first], tasks[t].second, (*rows)[tasks[t].first].data()); });
            }
            TIMED("w:hdf5");
            for (std::size_t r = 0; r < _R; r++) _stores[r]->save_contacts_packed(step, packed[r]);
        });
    }

    // advance to `target` and leave the state updates of callback(target) pending (GD_RUN_DEFER_CALLBACK): what the host
    // part of the reference's callback(target) sees -- mean_energy, the log line, the saved context and the contact search all
    // run BEFORE update_bead_scale() / update_wall_semiaxes() (simulation_driver_interphase.cc:20-43), i.e. on the scales, the
    // semiaxes and the contact distance that callback(target - 1) left
    void advance(gd_run_desc &run, long &step, long target)
    {
        run.steps = target - step; run.flags |= GD_RUN_DEFER_CALLBACK;
        { TIMED("gd_run"); chk(gd_run(_sys, &run)); }
        for (std::size_t r = 0; r < _R; r++) {
            gd_context ctx;
            chk(gd_get_context(_sys, (uint32_t)r, &ctx));
            _context[r].bead_scale = ctx.bead_scale; _context[r].bond_scale = ctx.bond_scale;
            std::copy(ctx.semiaxes, ctx.semiaxes + 3, _context[r].wall_semiaxes);
        }
        _contact_distance = _config.contactmap_distance * _context[0].bead_scale;     // set by update_bead_scale() of callback(target - 1), :66
                                                                                      // (replicas of one handle are at the same step: one scale)
        step = target;
    }

    void run_relaxation()
    {
        std::vector<double> xyz(3 * _n * _R);
        for (std::size_t r = 0; r < _R; r++) {
            _stores[r]->set_phase("relaxation");
            auto const init = _stores[r]->load_positions(0);
            if (init.size() != _n) throw std::runtime_error("relaxation/0/positions has the wrong number of beads");
            for (std::size_t i = 0; i < _n; i++) for (int k = 0; k < 3; k++) xyz[3 * (_n * r + i) + k] = init[i][k];
        }
        chk(gd_set_positions(_sys, xyz.data()));
        chk(gd_begin_phase(_sys, semiaxes().data()));
        auto callback = [&](long step) {
            bool const logging = step % _config.relaxation_logging_interval == 0, sampling = step % _config.relaxation_sampling_interval == 0;
            if (logging || sampling) mean_energy();
            if (logging) print_progress("relax", step);
            if (sampling) save_snapshot(step);
        };
        callback(0);
        std::vector<uint64_t> seeds(_R);
        for (std::size_t r = 0; r < _R; r++) seeds[r] = _random[r]();
        gd_run_desc run{};
        run.temperature = _config.relaxation_temperature; run.timestep = _config.relaxation_timestep;
        run.spacestep = _config.relaxation_spacestep; run.seed = seeds[0]; run.noise_mode = GD_NOISE_PHILOX; run.flags = 0;
        run.replica_seeds = _R > 1 ? seeds.data() : nullptr;
        long step = 0;
        while (step < _config.relaxation_steps) {
            long const next = std::min<long>(_config.relaxation_steps, std::min(next_multiple(step, _config.relaxation_logging_interval),
                                                                                next_multiple(step, _config.relaxation_sampling_interval)));
            run.steps = next - step; { TIMED("gd_run"); chk(gd_run(_sys, &run)); } step = next;
            callback(step);
        }
    }

    static long next_multiple(long step, long interval) { return (step / interval + 1) * interval; }

    void run_simulation()
    {
        { TIMED("writer_wait"); _writer.drain(); }          // (the relaxation's last snapshot goes to the relaxation phase)
        for (auto &st : _stores) st->set_phase("interphase");
        _interphase = true;
        double const dt = _config.interphase_timestep;
        chk(gd_begin_phase(_sys, semiaxes().data()));       // step = 0, time = 0
        std::vector<std::array<double, 3>> reaction(_R);
        for (std::size_t r = 0; r < _R; r++) {
            gd_context last;
            chk(gd_get_context(_sys, (uint32_t)r, &last));
            reaction[r] = {last.axial_reaction[0], last.axial_reaction[1], last.axial_reaction[2]};
        }

        // host part of callback(step): everything except the state updates that run on the device
        auto observe = [&](long step) {
            for (auto &c : _context) c.time = (double)step * dt;
            bool const logging = step % _config.interphase_logging_interval == 0, sampling = step % _config.interphase_sampling_interval == 0;
            long const frame = step / _config.interphase_sampling_interval;
            if (logging || sampling) mean_energy();
            if (logging) print_progress("inter", step);
            if (sampling) save_snapshot(step);
            if (step % _config.contactmap_update_interval == 0 && _contact_distance > 0) {   // (the reference's distance is 0 until callback(0) has set it)
                TIMED("contacts_update");
                chk(gd_contacts_update(_sys, _contact_distance));
            }
            if (sampling && frame % _config.contactmap_thinning_rate == 0) save_contacts(step);
        };

        // callback(0): observation, then update_bead_scale() and update_wall_semiaxes() on the host
        // (simulation_driver_interphase.cc:42-43,59-80); the packing reaction is that of the last force evaluation
        observe(0);
        double const spring[3] = {_config.wall_semiaxes_spring.x, _config.wall_semiaxes_spring.y, _config.wall_semiaxes_spring.z};
        for (std::size_t r = 0; r < _R; r++) {
            auto &c = _context[r];
            c.bead_scale = 1 - (1 - _config.bead_scale_init) * std::exp(-0.0 / _config.bead_scale_tau);
            c.bond_scale = 1 - (1 - _config.bond_scale_init) * std::exp(-0.0 / _config.bond_scale_tau);
            _contact_distance = _config.contactmap_distance * c.bead_scale;
            for (int k = 0; k < 3; k++)
                c.wall_semiaxes[k] += dt * _config.wall_mobility * (reaction[r][k] - spring[k] * c.wall_semiaxes[k]);
            chk(gd_set_context(_sys, (uint32_t)r, 0, c.bead_scale, c.bond_scale, c.wall_semiaxes));
        }

        std::vector<uint64_t> seeds(_R);
        for (std::size_t r = 0; r < _R; r++) seeds[r] = _random[r]();
        gd_run_desc run{};
        run.temperature = _config.interphase_temperature; run.timestep = dt; run.spacestep = _config.interphase_spacestep;
        run.seed = seeds[0]; run.noise_mode = GD_NOISE_PHILOX; run.flags = GD_RUN_UPDATE_SCALES | GD_RUN_WALL_DYNAMICS;
        run.replica_seeds = _R > 1 ? seeds.data() : nullptr;
        long step = 0;
        while (step < _config.interphase_steps) {
            long const next = std::min<long>(_config.interphase_steps,
                                             std::min({next_multiple(step, _config.interphase_logging_interval),
                                                       next_multiple(step, _config.interphase_sampling_interval),
                                                       next_multiple(step, _config.contactmap_update_interval)}));
            advance(run, step, next);
            observe(step);
            chk(gd_apply_callback(_sys));      // update_bead_scale() + update_wall_semiaxes() of callback(step), on the device
        }
    }

    std::vector<std::unique_ptr<gd::trajectory_store>> &_stores;
    std::size_t _R;
    gd::simulation_config _config;
    bool _auto_skin = false;
    ensemble_matrices *_ensemble = nullptr;
    flow_outputs *_flow = nullptr;
    model_classes const *_models = nullptr;
    bool _interphase = false;
    std::vector<gd::context> _context;
    double _contact_distance = 0;
    std::vector<std::mt19937_64> _random;
    gd_system *_sys = nullptr;
    std::size_t _n = 0;
    std::vector<float> _buffer;
    gd::thread_pool _pool{gd::usable_threads()};
    gd::async_writer _writer;      // (after the pool and the stores it uses: destroyed first)
    std::vector<double> _energy;
    unsigned long _energy_calls = 0, _energy_builds = 0;
    double _energy_max = 0;
};

}  // namespace

static bool is_flow_option(std::string const &arg)
{
    std::string const key = arg.substr(0, arg.find('='));
    for (char const *k : {"--scan-radius", "--smoothing", "--velocity-delay", "--name", "--grid-interval", "--x-range", "--y-range", "--z-range"})
        if (key == k) return true;
    return false;
}

int main(int argc, char **argv)
{
    // gd_interphase <trajectory> [device]                      the reference's command line
    // gd_interphase [--device d] <trajectory> <trajectory>...  R prepared files as R replicas of one handle
    // options: --timing (wall-time split on stderr at the end), --auto-skin (list width selected from measured chunk times: the
    // trajectory of a seed then depends on timing; off by default.  --fixed-skin, the former spelling of the default, is accepted),
    // --ensemble-matrix RATE OUTPUT (the genome-wide contact matrix of the replicas, as gd_gw_contact_matrix --rebin-rate RATE writes it;
    // files that differ in their A/B factors form models: OUTPUT then needs {model}, and every model gets its own matrix),
    // --particle-flow OUTPUT / --grid-flow OUTPUT with the options of gd_particle_flow / gd_grid_flow: --scan-radius, --smoothing,
    // --velocity-delay, --name, and for the grid --grid-interval, --x-range, --y-range, --z-range (per replica: a batch of several
    // models needs nothing else)
    std::vector<std::string> files, flow_args;
    std::string particle_output, grid_output;
    bool particle_asked = false, grid_asked = false;
    std::string matrix_output;
    long matrix_rate = 0;
    int device = 0;
    bool timing = false, auto_skin = false;
    auto const t_start = std::chrono::steady_clock::now();
    for (int i = 1; i < argc; i++) {
        std::string const arg = argv[i];
        if (arg == "--timing") timing = true;
        else if (arg == "--auto-skin") auto_skin = true;
        else if (arg == "--fixed-skin") auto_skin = false;
        else if (arg == "--device" && i + 1 < argc) device = std::stoi(argv[++i]);
        else if (arg == "--ensemble-matrix") {
            char *end = nullptr;
            if (i + 2 < argc) matrix_rate = std::strtol(argv[i + 1], &end, 10);
            if (i + 2 >= argc || *end || matrix_rate < 1) {
                std::cerr << "error: --ensemble-matrix takes a rebin rate of at least 1 and an output file\n";
                return 1;
            }
            matrix_output = argv[i + 2];
            i += 2;
        }
        else if (arg == "--particle-flow" || arg == "--grid-flow") {
            bool const grid = arg == "--grid-flow";
            (grid ? grid_asked : particle_asked) = true;
            if (i + 1 < argc) (grid ? grid_output : particle_output) = argv[++i];
        }
        else if (is_flow_option(arg)) {
            flow_args.push_back(arg);
            if (arg.find('=') == std::string::npos && i + 1 < argc) flow_args.push_back(argv[++i]);
        }
        else files.push_back(arg);
    }
    if ((particle_asked || grid_asked) && !flow_outputs::available()) {
        std::cerr << "error: " << (particle_asked ? "--particle-flow" : "--grid-flow") << " needs the device library\n";
        return 1;
    }
    if ((particle_asked && particle_output.empty()) || (grid_asked && grid_output.empty())) {
        std::cerr << "error: --particle-flow and --grid-flow take an output file\n";
        return 1;
    }
    if (!flow_args.empty() && !particle_asked && !grid_asked) {
        std::cerr << "error: " << flow_args[0] << " needs --particle-flow or --grid-flow\n";
        return 1;
    }
    if (!matrix_output.empty() && !ensemble_matrix::available()) {
        std::cerr << "error: --ensemble-matrix needs the device library\n";
        return 1;
    }
    if (files.size() == 2 && !files[1].empty() && files[1].find_first_not_of("0123456789") == std::string::npos) {
        device = std::stoi(files[1]); files.pop_back();
    }
    if (files.empty()) {
        std::cerr << "usage: gd_interphase <trajectory> [device]\n       gd_interphase [--device d] <trajectory> <trajectory>...\n"
                     "files that differ in their A/B factors alone run as the models of one batch; --ensemble-matrix RATE OUTPUT then writes one\n"
                     "matrix per model and OUTPUT must contain {model}; --particle-flow / --grid-flow work per replica and need no change\n";
        return 1;
    }
    std::unique_ptr<flow_outputs> flow;
    if (particle_asked || grid_asked) {      // the shared flow options, parsed once per analysis as its own program parses them
        flow = std::make_unique<flow_outputs>();
        std::vector<char *> av = {argv[0]};
        for (auto &a : flow_args) av.push_back(a.data());
        for (int grid = 0; grid < 2; grid++) {
            if (!(grid ? grid_asked : particle_asked)) continue;
            gd::flow::options &o = grid ? flow->grid : flow->particle;
            std::string err;
            std::string out = grid ? grid_output : particle_output, dummy = "trajfile";
            std::vector<char *> full = av;
            full.push_back(out.data());
            full.push_back(dummy.data());
            if (gd::flow::parse((int)full.size(), full.data(), grid != 0, o, err, grid_asked)) {
                std::cerr << "error: " << err << '\n';
                return 1;
            }
            if (o.delay < 0 || o.smoothing < 0) {
                std::cerr << "error: --velocity-delay and --smoothing must be >= 0\n";
                return 1;
            }
        }
    }
    try {
        // the models of the batch, from the files' factors -- before a file is opened for writing, so that a refused command line leaves
        // every file as it was
        model_classes models;      // (one file: the reference's command line, one model)
        if (files.size() > 1) models = classify_models(files);
        else { models.of = {0}; models.n = 1; }
        bool const per_model = models.n > 1 && gd_ensemble_set_ab && gd_ensemble_classes;      // (else: the set-up refuses the batch)
        if (per_model && !matrix_output.empty() && matrix_output.find("{model}") == std::string::npos) {
            std::cerr << "error: the files hold " << models.n << " models (their A/B factors differ): the output of --ensemble-matrix must contain {model}\n";
            return 1;
        }
        if (per_model)
            for (uint32_t k = 0; k < models.n; k++) {
                std::clog << "[model " << k << "]";
                for (auto const &f : models.files_of(files, k)) std::clog << " file " << f;
                std::clog << '\n';
            }
        std::unique_ptr<ensemble_matrices> ensemble;      // (reads the chromosome tables before the stores open the files)
        if (!matrix_output.empty()) ensemble = std::make_unique<ensemble_matrices>(files, models, matrix_rate, matrix_output, device);
        std::vector<std::unique_ptr<gd::trajectory_store>> stores;
        {
            TIMED("open_files");
            for (auto const &f : files) stores.push_back(std::make_unique<gd::trajectory_store>(f));
        }
        double bead_steps = 0;
        {
            simulation_driver driver{stores, device, auto_skin, ensemble.get(), flow.get(), &models};
            driver.run();
            bead_steps = driver.bead_steps();
            if (ensemble) { TIMED("ensemble_matrix"); ensemble->write(); }
            if (flow) {
                TIMED("flow_outputs");
                // the stand-alone programs read every stored frame: a file that held interphase snapshots before this run has more
                // of them than were recorded
                for (std::size_t r = 0; r < stores.size(); r++)
                    if (stores[r]->load_steps().size() != flow->frames())
                        throw std::runtime_error(files[r] + " holds " + std::to_string(stores[r]->load_steps().size()) + " interphase snapshots, " +
                                                 std::to_string(flow->frames()) + " were recorded in this run: the flow outputs are not written");
                flow->write(files, device);
            }
        }
        { TIMED("close_files"); stores.clear(); }
        double const total_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
        g_timing.add("total", total_s);
        // a batched run (the farm's unit: one process per GPU) reports its device's rate, files opened to files closed -- the first
        // 8-GPU run of gd_farm yields the scaling table from these lines alone (a solo run keeps the reference's output)
        if (files.size() > 1 || timing)
            std::clog << "[rate] device " << device << ": " << files.size() << " file(s), " << bead_steps << " bead-steps in " << total_s << " s = "
                      << bead_steps / total_s << " bead-steps/s\n";
        if (timing) g_timing.print();
    } catch (std::exception const &e) {
        std::cerr << "error: " << e.what() << '\n';
        return 1;
    }
    return 0;
}
