// gd_1kb -- the 1 kb-resolution chromatin loop-formation driver on libgdyn.
//
// Mirrors the reference program `main [-hCos] <config>` of 3-sim-1kb/src/simulation (main.cpp:40-186,
// simulation.cpp:37-305, topology.cpp:6-21, loops.cpp:12-92, glues.cpp:4-17, inits.cpp:10-22,
// inits/box_initializer.cpp:18-38, inits/utils.hpp:9-47, store.cpp:17-58): same JSON configuration, same
// command-line options, same log lines, same output datasets.  The Brownian dynamics runs on the device in chunks
// that end at the next logging / sampling / loop-update / glue-update step; the loop and glue lists are the
// re-uploadable pair slots of the C-ABI (the reference's custom md::forcefield subclasses, forces/loop_forcefield.cpp,
// forces/glue_forcefield.cpp); loop extrusion and glue kinetics stay on the host on std::mt19937_64
// (gd_1kb_kinetics.hpp), the glue candidate search uses the device cell list (gd_search_pairs).
//
// Options beyond the reference's: -d <device>; --trace <dir> (test support): writes <dir>/init.f64 (initial positions) and
// <dir>/trace.txt with the integrator seed and every loop / glue list uploaded, so a run can be replayed call by call;
// --auto-skin: let the library select the list width from measured chunk times (gd_tuning.auto_skin).  Off by default: the
// selection changes cost only, but it reads a clock -- the cell decomposition, and with it the fp32 summation order of a
// trajectory, would differ from run to run, where the reference gives one trajectory per seed.  (--fixed-skin, the former
// spelling of the default, is still accepted.)
// --seeds s0,s1,...: an ensemble of trajectories as the replicas of ONE handle (class ensemble below): replica r is the trajectory
// `-s s_r` would start, with its own generator, kinetics, output file (the output name holds the placeholder {seed}) and trace
// (<dir>/seed-<s_r>/).  Its loops and glues are the per-replica pair lists of include/gdyn_replica.h, which only libgdyn has: the
// symbols are referenced weakly, and two or more seeds are refused where they are absent.  One seed runs exactly as -s.
// --device-glues (with --seeds, one seed or more): the glue kinetics of all trajectories in one device call per update
// (gd_glue_update, include/gdyn_glue.h) instead of a position download, two pair searches and one generator
// draw per candidate on the host for every trajectory.  The same stochastic process with counter-based draws keyed by the
// trajectory's seed: deterministic, but not the reference's mt19937_64 sequence, which the default keeps draw for draw.
// The program reads no environment variable.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <memory>
#include <optional>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/gdyn.h"
#include "../../include/gdyn_replica.h"
// This program is also linked against libraries that implement gdyn.h alone (the fp64 oracle of the tests): what --seeds calls is
// referenced weakly, and an ensemble is refused where the symbols are absent.
#pragma weak gd_replica_pairs_define
#pragma weak gd_replica_pairs_set
#include "../../include/gdyn_glue.h"
#pragma weak gd_glue_define
#pragma weak gd_glue_update
#pragma weak gd_glue_fetch
#pragma weak gd_glue_counts
#include "gd_1kb_config.hpp"
#include "gd_1kb_kinetics.hpp"
#include "gd_1kb_store.hpp"

namespace {

using namespace gd1kb;

void chk(int rc) { if (rc != GD_OK) throw std::runtime_error(gd_last_error()); }

struct chain_assignment { std::size_t start = 0, end = 0; chain_config const *config = nullptr; };

std::vector<chain_assignment> make_chain_assignments(simulation_config const &config)      // topology.cpp:6-21
{
    std::vector<chain_assignment> out;
    std::size_t offset = 0;
    for (auto const &chain : config.chains) {
        out.push_back({offset, offset + chain.length, &chain});
        offset += chain.length;
    }
    return out;
}

std::mt19937_64 make_random(std::uint64_t seed)      // simulation.cpp:29-34
{
    std::seed_seq seq{seed};
    return std::mt19937_64{seq};
}

// one virtual lattice over the concatenated chains; boundaries stop factors from hopping across (loops.cpp:12-92)
gd::loop_extruder make_loop_extruder(simulation_config const &config, std::vector<chain_assignment> const &chains)
{
    std::size_t length = 0, max_loops = 0;
    for (auto const &c : chains) length += c.config->length;
    if (config.loop.max_loops) max_loops = *config.loop.max_loops;
    else for (auto const &c : chains) max_loops += c.config->loaded_loops.size();
    gd::loop_extruder loops{length, max_loops};
    loops.set_forward_speed(config.loop.forward_speed);
    loops.set_backward_speed(config.loop.backward_speed);
    loops.set_loading_rate(config.loop.loading_rate_density * double(length));
    loops.set_unloading_rate(config.loop.unloading_rate);
    if (config.loop.crossing_rate) loops.set_crossing_rate(*config.loop.crossing_rate);
    for (auto const &c : chains) {
        for (auto pos : c.config->forward_boundaries) {        // factors stall on the right neighbour
            loops.add_boundary(c.start + pos);
            if (c.start + pos + 1 < c.end) loops.set_site_detachability(c.start + pos + 1, config.loop.convergent_detachability);
        }
        for (auto pos : c.config->backward_boundaries) {       // ... and on the left neighbour
            loops.add_boundary(c.start + pos);
            if (c.start + pos >= c.start + 1) loops.set_site_detachability(c.start + pos - 1, config.loop.convergent_detachability);
        }
        for (auto pos : c.config->roadblocks) loops.set_site_attachability(c.start + pos, config.loop.roadblock_attachability);
    }
    for (auto const &c : chains)
        for (auto pos : c.config->loaded_loops) loops.load_loop(c.start + pos);
    return loops;
}

class simulation {
public:
    simulation(simulation_config const &config, int device, std::string const &trace_dir = "", bool auto_skin = false)
        : _config(config), _random(make_random(config.sampling.random_seed)), _store(config.sampling.output_filename),
          _chains(make_chain_assignments(_config)), _loops(make_loop_extruder(_config, _chains)),
          _glues(_config.glue.max_glues, _config.glue.glue_distance, _config.glue.glue_binding_rate, _config.glue.glue_unbinding_rate,
                 _config.chain.box_size)
    {
        for (auto const &c : _chains) _n += c.config->length;
        if (_n == 0) throw std::runtime_error("no monomers: the configuration defines no chains");
        _auto_skin = auto_skin;
        if (!trace_dir.empty()) { _trace_dir = trace_dir; _trace.open(_trace_dir + "/trace.txt"); }
        setup_system(device);
        std::vector<int> ranges;
        for (auto const &c : _chains) { ranges.push_back(int(c.start)); ranges.push_back(int(c.end)); }
        _store.save_metadata(format_simulation_config(_config), _config.config_text, ranges);
    }
    ~simulation() { gd_destroy(_sys); }

    void run()
    {
        initialize_particles();
        if (_config.sampling.loop_preloading) _loops.preload(_random);
        run_simulation();
    }

private:
    // particles + force fields (simulation.cpp:57-186)
    void setup_system(int device)
    {
        auto const &ch = _config.chain;
        gd_desc desc{};
        desc.n_beads = (uint32_t)_n; desc.n_replicas = 1; desc.device = device; desc.box_kind = GD_BOX_PERIODIC;
        desc.box[0] = desc.box[1] = desc.box[2] = ch.box_size;
        chk(gd_create(&desc, &_sys));
        {   // the list width: the library's state-based default, or (--auto-skin) selected from measured chunk times
            gd_tuning tune{};
            tune.adapt_interval = 1; tune.auto_skin = _auto_skin ? 1 : 0;
            chk(gd_set_tuning(_sys, &tune));
        }
        std::vector<double> mobility(_n, ch.monomer_mobility), bending(_n, ch.bending_energy);
        for (auto const &c : _chains)
            for (auto const &block : c.config->blocks)
                for (std::size_t i = block.start; i < block.end; i++)
                    if (block.bending_energy) bending.at(c.start + i) = *block.bending_energy;
        chk(gd_set_bead_params(_sys, nullptr, nullptr, mobility.data(), bending.data()));
        gd_pair_softcore pair{};      // softcore<2,3>{rep} + softcore<8,3>{-attr}, unmixed
        pair.eps_a = ch.repulsive_energy; pair.sigma_a = ch.repulsive_diameter; pair.p_a = 2; pair.q_a = 3;
        pair.eps_b = ch.attractive_energy * -1; pair.sigma_b = ch.attractive_diameter; pair.p_b = 8; pair.q_b = 3;
        chk(gd_set_pair_softcore(_sys, &pair));
        gd_bond_params bond{};
        bond.kind = GD_POT_SPRING; bond.k_a = ch.bond_spring; bond.l_a = ch.bond_length;
        for (auto const &c : _chains) {
            chk(gd_add_bond_range(_sys, &bond, (uint32_t)c.start, (uint32_t)c.end, 1));
            chk(gd_add_bending_range(_sys, (uint32_t)c.start, (uint32_t)c.end, 0.0, /*per_bead=*/1));
        }
        _loop_bond.kind = GD_POT_SPRING; _loop_bond.k_a = _config.loop.bond_spring; _loop_bond.l_a = ch.repulsive_diameter;
        _glue_bond.kind = GD_POT_SOFTCORE; _glue_bond.k_a = -_config.glue.glue_energy; _glue_bond.l_a = _config.glue.glue_distance;
        _glue_bond.p = 8; _glue_bond.q = 3; _glue_bond.minimum_image = 1;
    }

    // chain centroids uniform in the box, one continuous random walk over all monomers, then every chain is shifted
    // onto its centroid (inits/box_initializer.cpp:18-38, inits/utils.hpp:9-47)
    void initialize_particles()
    {
        auto const &ch = _config.chain;
        std::vector<double> centroids;
        for (std::size_t c = 0; c < _chains.size(); c++) {
            std::uniform_real_distribution<double> coord{0, ch.box_size};
            for (int k = 0; k < 3; k++) centroids.push_back(coord(_random));
        }
        _xyz.assign(3 * _n, 0.0);
        double walk[3] = {0, 0, 0};
        for (std::size_t i = 0; i < _n; i++) {
            for (int k = 0; k < 3; k++) _xyz[3 * i + k] = walk[k];
            std::normal_distribution<double> normal;
            double d[3] = {normal(_random), normal(_random), normal(_random)};
            double const inv = 1 / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; k++) walk[k] += ch.initial_bond_length * (d[k] * inv);
        }
        for (std::size_t c = 0; c < _chains.size(); c++) {
            auto const &chain = _chains[c];
            double offset[3] = {0, 0, 0};
            for (std::size_t i = chain.start; i < chain.end; i++)
                for (int k = 0; k < 3; k++) offset[k] += _xyz[3 * i + k] - centroids[3 * c + k];
            for (int k = 0; k < 3; k++) offset[k] /= double(chain.end - chain.start);
            for (std::size_t i = chain.start; i < chain.end; i++)
                for (int k = 0; k < 3; k++) _xyz[3 * i + k] -= offset[k];
        }
        chk(gd_set_positions(_sys, _xyz.data()));
        if (!_trace_dir.empty()) {
            std::ofstream out(_trace_dir + "/init.f64", std::ios::binary);
            out.write(reinterpret_cast<char const *>(_xyz.data()), (std::streamsize)(_xyz.size() * sizeof(double)));
        }
    }

    void upload_loops(long step)
    {
        // a freshly loaded factor holds a zero-length loop (start == end): no force, the constant energy K b^2 / 2 of
        // the spring at r = 0; the pair slot takes distinct beads only, so that constant is added in show_progress
        std::vector<uint32_t> pairs;
        _zero_length_loops = 0;
        for (auto const &l : _loops.loops()) {
            if (!l.id) continue;
            if (l.start == l.end) { _zero_length_loops++; continue; }
            pairs.push_back((uint32_t)l.start); pairs.push_back((uint32_t)l.end);
        }
        chk(gd_set_dynamic_pairs(_sys, 0, &_loop_bond, pairs.data(), (uint32_t)(pairs.size() / 2)));
        trace("loops", step, pairs);
    }

    void upload_glues(long step)
    {
        std::vector<std::pair<uint32_t, uint32_t>> sorted;
        for (auto const &g : _glues.pairs()) sorted.push_back({g.i, g.j});
        std::sort(sorted.begin(), sorted.end());
        std::vector<uint32_t> pairs;
        for (auto const &g : sorted) { pairs.push_back(g.first); pairs.push_back(g.second); }
        chk(gd_set_dynamic_pairs(_sys, 1, &_glue_bond, pairs.data(), (uint32_t)(pairs.size() / 2)));
        trace("glues", step, pairs);
    }

    void trace(char const *what, long step, std::vector<uint32_t> const &pairs)
    {
        if (!_trace.is_open()) return;
        _trace << what << ' ' << step << ' ' << pairs.size() / 2;
        for (auto v : pairs) _trace << ' ' << v;
        _trace << '\n' << std::flush;
    }

    // simulation.cpp:245-260
    void step_loops(long step)
    {
        auto const &s = _config.sampling;
        double const leap = s.timestep * double(s.loop_update_interval);
        if (!s.clear_loops_at || step < s.clear_loops_at) _loops.step(leap, _random);
        if (step + 1 == s.clear_loops_at) _loops.clear();
        upload_loops(step);
    }

    // simulation.cpp:263-270; candidates come from the device cell list
    void step_glues(long step)
    {
        if (!_glues.enabled()) return;
        auto const &s = _config.sampling;
        double const leap = s.timestep * double(s.glue_update_interval);
        chk(gd_get_positions(_sys, _xyz.data()));
        uint64_t n = 0;
        chk(gd_search_pairs(_sys, 0, _glues.reach(), nullptr, 0, &n));
        std::vector<uint32_t> candidates(2 * n);
        if (n) chk(gd_search_pairs(_sys, 0, _glues.reach(), candidates.data(), n, &n));
        _glues.update(leap, _xyz.data(), candidates, _random);
        upload_glues(step);
    }

    // "step \t E: .. \t L: .. \t G: .." (simulation.cpp:273-296)
    void show_progress(long step)
    {
        double e = 0;
        chk(gd_compute_energy(_sys, GD_TERM_ALL, &e));
        e += double(_zero_length_loops) * 0.5 * _loop_bond.k_a * _loop_bond.l_a * _loop_bond.l_a;
        double const n = double(_n);
        std::clog << step << '\t' << "E: " << e / n << '\t' << "L: " << double(_loops.loaded()) / n << '\t'
                  << "G: " << double(_glues.size()) / n << '\n';
    }

    void save_sample()
    {
        chk(gd_get_positions(_sys, _xyz.data()));
        std::vector<long long> loops;
        for (auto const &l : _loops.loops()) { loops.push_back((long long)l.start); loops.push_back((long long)l.end); loops.push_back((long long)l.id); }
        _store.save_snapshot(_xyz.data(), _n, loops);
    }

    static long next_multiple(long step, long interval) { return (step / interval + 1) * interval; }

    // simulation.cpp:212-242
    void run_simulation()
    {
        auto const &s = _config.sampling;
        for (long interval : {s.logging_interval, s.sampling_interval, s.loop_update_interval, s.glue_update_interval})
            if (interval <= 0) throw std::runtime_error("intervals must be positive");
        auto callback = [&](long step) {
            if (step % s.logging_interval == 0) show_progress(step);
            if (step % s.sampling_interval == 0) save_sample();
            if (step % s.loop_update_interval == 0) step_loops(step);
            if (step % s.glue_update_interval == 0) step_glues(step);
        };
        chk(gd_begin_phase(_sys, nullptr));
        upload_loops(-1);                 // the initially loaded / preloaded loops act from the first energy evaluation on
        callback(0);
        gd_run_desc run{};
        run.temperature = s.temperature; run.timestep = s.timestep; run.seed = _random(); run.noise_mode = GD_NOISE_PHILOX;
        if (_trace.is_open()) _trace << "seed " << run.seed << '\n' << std::flush;
        long step = 0;
        while (step < s.steps) {
            long const next = std::min<long>(s.steps, std::min({next_multiple(step, s.logging_interval), next_multiple(step, s.sampling_interval),
                                                               next_multiple(step, s.loop_update_interval), next_multiple(step, s.glue_update_interval)}));
            run.steps = next - step; chk(gd_run(_sys, &run)); step = next;
            callback(step);
        }
    }

    simulation_config _config;
    std::mt19937_64 _random;         // shared by the initialiser, loop preloading, the integrator seed and all kinetics
    history_store _store;
    std::vector<chain_assignment> _chains;
    gd::loop_extruder _loops;
    gd::glue_binder _glues;
    gd_system *_sys = nullptr;
    std::size_t _n = 0, _zero_length_loops = 0;
    gd_bond_params _loop_bond{}, _glue_bond{};
    std::vector<double> _xyz;
    std::string _trace_dir;
    std::ofstream _trace;
    bool _auto_skin = false;
};

// --seeds: K trajectories as the replicas of one handle.  Every member function is simulation's, per replica: the same draws from the
// replica's own generator in the same order, the same log lines (prefixed "[seed s]"), the same datasets in the replica's own file.
class ensemble {
public:
    ensemble(simulation_config const &config, std::vector<std::uint64_t> const &seeds, std::vector<std::string> const &outputs, int device,
             std::string const &trace_dir, bool auto_skin, bool device_glues = false)
        : _config(config), _chains(make_chain_assignments(_config)), _auto_skin(auto_skin), _device_glues(device_glues)
    {
        for (auto const &c : _chains) _n += c.config->length;
        if (_n == 0) throw std::runtime_error("no monomers: the configuration defines no chains");
        std::vector<int> ranges;
        for (auto const &c : _chains) { ranges.push_back(int(c.start)); ranges.push_back(int(c.end)); }
        for (std::size_t r = 0; r < seeds.size(); r++) {
            simulation_config own = _config;      // what `-s s_r -o <its file>` would run with
            own.sampling.random_seed = seeds[r]; own.sampling.output_filename = outputs[r];
            _replicas.push_back(std::make_unique<replica>(own, _chains));
            auto &t = *_replicas.back();
            if (!trace_dir.empty()) {
                t.trace_dir = trace_dir + "/seed-" + std::to_string(seeds[r]);
                std::filesystem::create_directories(t.trace_dir);
                t.trace.open(t.trace_dir + "/trace.txt");
            }
            t.store.save_metadata(format_simulation_config(own), own.config_text, ranges);
        }
        setup_system(device);
    }
    ~ensemble() { gd_destroy(_sys); }

    void run()
    {
        _xyz.assign(3 * _n * _replicas.size(), 0.0);
        for (std::size_t r = 0; r < _replicas.size(); r++) initialize_particles(r);
        chk(gd_set_positions(_sys, _xyz.data()));
        if (_config.sampling.loop_preloading) for (auto &t : _replicas) t->loops.preload(t->random);
        run_simulation();
    }

private:
    struct replica {
        replica(simulation_config const &own, std::vector<chain_assignment> const &chains)
            : seed(own.sampling.random_seed), random(make_random(seed)), store(own.sampling.output_filename),
              loops(make_loop_extruder(own, chains)),
              glues(own.glue.max_glues, own.glue.glue_distance, own.glue.glue_binding_rate, own.glue.glue_unbinding_rate, own.chain.box_size)
        {
        }
        std::uint64_t seed;
        std::mt19937_64 random;      // shared by this trajectory's initialiser, loop preloading, integrator seed and kinetics
        history_store store;
        gd::loop_extruder loops;
        gd::glue_binder glues;
        std::size_t zero_length_loops = 0;
        std::string trace_dir;
        std::ofstream trace;
    };

    // simulation::setup_system with K replicas; the loop and glue sets are per-replica slots 0 and 1
    void setup_system(int device)
    {
        auto const &ch = _config.chain;
        gd_desc desc{};
        desc.n_beads = (uint32_t)_n; desc.n_replicas = (uint32_t)_replicas.size(); desc.device = device; desc.box_kind = GD_BOX_PERIODIC;
        desc.box[0] = desc.box[1] = desc.box[2] = ch.box_size;
        chk(gd_create(&desc, &_sys));
        {
            gd_tuning tune{};
            tune.adapt_interval = 1; tune.auto_skin = _auto_skin ? 1 : 0;
            chk(gd_set_tuning(_sys, &tune));
        }
        std::vector<double> mobility(_n, ch.monomer_mobility), bending(_n, ch.bending_energy);
        for (auto const &c : _chains)
            for (auto const &block : c.config->blocks)
                for (std::size_t i = block.start; i < block.end; i++)
                    if (block.bending_energy) bending.at(c.start + i) = *block.bending_energy;
        chk(gd_set_bead_params(_sys, nullptr, nullptr, mobility.data(), bending.data()));
        gd_pair_softcore pair{};
        pair.eps_a = ch.repulsive_energy; pair.sigma_a = ch.repulsive_diameter; pair.p_a = 2; pair.q_a = 3;
        pair.eps_b = ch.attractive_energy * -1; pair.sigma_b = ch.attractive_diameter; pair.p_b = 8; pair.q_b = 3;
        chk(gd_set_pair_softcore(_sys, &pair));
        gd_bond_params bond{};
        bond.kind = GD_POT_SPRING; bond.k_a = ch.bond_spring; bond.l_a = ch.bond_length;
        for (auto const &c : _chains) {
            chk(gd_add_bond_range(_sys, &bond, (uint32_t)c.start, (uint32_t)c.end, 1));
            chk(gd_add_bending_range(_sys, (uint32_t)c.start, (uint32_t)c.end, 0.0, /*per_bead=*/1));
        }
        _loop_bond.kind = GD_POT_SPRING; _loop_bond.k_a = _config.loop.bond_spring; _loop_bond.l_a = ch.repulsive_diameter;
        _glue_bond.kind = GD_POT_SOFTCORE; _glue_bond.k_a = -_config.glue.glue_energy; _glue_bond.l_a = _config.glue.glue_distance;
        _glue_bond.p = 8; _glue_bond.q = 3; _glue_bond.minimum_image = 1;
        chk(gd_replica_pairs_define(_sys, 0, &_loop_bond));
        chk(gd_replica_pairs_define(_sys, 1, &_glue_bond));
        if (_device_glues && _config.glue.max_glues != 0) {      // slot 1's lists come from the device kinetics
            gd_glue_params glue{};
            glue.max_glues = (uint32_t)_config.glue.max_glues; glue.reach = _config.glue.glue_distance;
            glue.binding_rate = _config.glue.glue_binding_rate; glue.unbinding_rate = _config.glue.glue_unbinding_rate;
            chk(gd_glue_define(_sys, 1, &glue));
            _glue_counts.assign(_replicas.size(), 0);
        }
    }

    double *xyz(std::size_t r) { return _xyz.data() + 3 * _n * r; }

    // simulation::initialize_particles on replica r's generator, into its part of the positions
    void initialize_particles(std::size_t r)
    {
        auto const &ch = _config.chain;
        auto &random = _replicas[r]->random;
        double *x = xyz(r);
        std::vector<double> centroids;
        for (std::size_t c = 0; c < _chains.size(); c++) {
            std::uniform_real_distribution<double> coord{0, ch.box_size};
            for (int k = 0; k < 3; k++) centroids.push_back(coord(random));
        }
        double walk[3] = {0, 0, 0};
        for (std::size_t i = 0; i < _n; i++) {
            for (int k = 0; k < 3; k++) x[3 * i + k] = walk[k];
            std::normal_distribution<double> normal;
            double d[3] = {normal(random), normal(random), normal(random)};
            double const inv = 1 / std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; k++) walk[k] += ch.initial_bond_length * (d[k] * inv);
        }
        for (std::size_t c = 0; c < _chains.size(); c++) {
            auto const &chain = _chains[c];
            double offset[3] = {0, 0, 0};
            for (std::size_t i = chain.start; i < chain.end; i++)
                for (int k = 0; k < 3; k++) offset[k] += x[3 * i + k] - centroids[3 * c + k];
            for (int k = 0; k < 3; k++) offset[k] /= double(chain.end - chain.start);
            for (std::size_t i = chain.start; i < chain.end; i++)
                for (int k = 0; k < 3; k++) x[3 * i + k] -= offset[k];
        }
        if (!_replicas[r]->trace_dir.empty()) {
            std::ofstream out(_replicas[r]->trace_dir + "/init.f64", std::ios::binary);
            out.write(reinterpret_cast<char const *>(x), (std::streamsize)(3 * _n * sizeof(double)));
        }
    }

    void upload_loops(std::size_t r, long step)
    {
        auto &t = *_replicas[r];
        std::vector<uint32_t> pairs;
        t.zero_length_loops = 0;      // (a zero-length loop: no force, a constant energy added in show_progress)
        for (auto const &l : t.loops.loops()) {
            if (!l.id) continue;
            if (l.start == l.end) { t.zero_length_loops++; continue; }
            pairs.push_back((uint32_t)l.start); pairs.push_back((uint32_t)l.end);
        }
        chk(gd_replica_pairs_set(_sys, 0, (uint32_t)r, pairs.data(), (uint32_t)(pairs.size() / 2)));
        trace(t, "loops", step, pairs);
    }

    void upload_glues(std::size_t r, long step)
    {
        auto &t = *_replicas[r];
        std::vector<std::pair<uint32_t, uint32_t>> sorted;
        for (auto const &g : t.glues.pairs()) sorted.push_back({g.i, g.j});
        std::sort(sorted.begin(), sorted.end());
        std::vector<uint32_t> pairs;
        for (auto const &g : sorted) { pairs.push_back(g.first); pairs.push_back(g.second); }
        chk(gd_replica_pairs_set(_sys, 1, (uint32_t)r, pairs.data(), (uint32_t)(pairs.size() / 2)));
        trace(t, "glues", step, pairs);
    }

    static void trace(replica &t, char const *what, long step, std::vector<uint32_t> const &pairs)
    {
        if (!t.trace.is_open()) return;
        t.trace << what << ' ' << step << ' ' << pairs.size() / 2;
        for (auto v : pairs) t.trace << ' ' << v;
        t.trace << '\n' << std::flush;
    }

    void step_loops(long step)
    {
        auto const &s = _config.sampling;
        double const leap = s.timestep * double(s.loop_update_interval);
        for (std::size_t r = 0; r < _replicas.size(); r++) {
            auto &t = *_replicas[r];
            if (!s.clear_loops_at || step < s.clear_loops_at) t.loops.step(leap, t.random);
            if (step + 1 == s.clear_loops_at) t.loops.clear();
            upload_loops(r, step);
        }
    }

    void step_glues(long step)
    {
        if (!_replicas[0]->glues.enabled()) return;
        auto const &s = _config.sampling;
        double const leap = s.timestep * double(s.glue_update_interval);
        if (_device_glues) { step_glues_on_device(step, leap); return; }
        chk(gd_get_positions(_sys, _xyz.data()));
        for (std::size_t r = 0; r < _replicas.size(); r++) {
            auto &t = *_replicas[r];
            uint64_t n = 0;
            chk(gd_search_pairs(_sys, (uint32_t)r, t.glues.reach(), nullptr, 0, &n));
            std::vector<uint32_t> candidates(2 * n);
            if (n) chk(gd_search_pairs(_sys, (uint32_t)r, t.glues.reach(), candidates.data(), n, &n));
            t.glues.update(leap, xyz(r), candidates, t.random);
            upload_glues(r, step);
        }
    }

    // --device-glues: one update of every trajectory on the device, keyed by the trajectory's seed and the update's number; the new
    // lists are in slot 1 when it returns.  Only the set sizes come back, and the sets themselves when a trace is written.
    void step_glues_on_device(long step, double leap)
    {
        std::vector<uint64_t> seeds;
        for (auto const &t : _replicas) seeds.push_back(t->seed);
        chk(gd_glue_update(_sys, leap, uint64_t(step / _config.sampling.glue_update_interval), seeds.data()));
        chk(gd_glue_counts(_sys, _glue_counts.data()));
        for (std::size_t r = 0; r < _replicas.size(); r++) {
            auto &t = *_replicas[r];
            if (!t.trace.is_open()) continue;
            std::vector<uint32_t> pairs(2 * std::size_t(_glue_counts[r]));
            uint32_t n = 0;
            chk(gd_glue_fetch(_sys, (uint32_t)r, pairs.data(), _glue_counts[r], &n));
            trace(t, "glues", step, pairs);
        }
    }

    // one line per replica: "[seed s] step \t E: .. \t L: .. \t G: .."
    void show_progress(long step)
    {
        std::vector<double> e(_replicas.size(), 0.0);
        chk(gd_compute_energy(_sys, GD_TERM_ALL, e.data()));
        double const n = double(_n);
        for (std::size_t r = 0; r < _replicas.size(); r++) {
            auto const &t = *_replicas[r];
            double const er = e[r] + double(t.zero_length_loops) * 0.5 * _loop_bond.k_a * _loop_bond.l_a * _loop_bond.l_a;
            std::clog << "[seed " << t.seed << "] " << step << '\t' << "E: " << er / n << '\t' << "L: " << double(t.loops.loaded()) / n << '\t'
                      << "G: " << double(_glue_counts.empty() ? t.glues.size() : std::size_t(_glue_counts[r])) / n << '\n';
        }
    }

    void save_sample()
    {
        chk(gd_get_positions(_sys, _xyz.data()));
        for (std::size_t r = 0; r < _replicas.size(); r++) {
            auto &t = *_replicas[r];
            std::vector<long long> loops;
            for (auto const &l : t.loops.loops()) { loops.push_back((long long)l.start); loops.push_back((long long)l.end); loops.push_back((long long)l.id); }
            t.store.save_snapshot(xyz(r), _n, loops);
        }
    }

    static long next_multiple(long step, long interval) { return (step / interval + 1) * interval; }

    void run_simulation()
    {
        auto const &s = _config.sampling;
        for (long interval : {s.logging_interval, s.sampling_interval, s.loop_update_interval, s.glue_update_interval})
            if (interval <= 0) throw std::runtime_error("intervals must be positive");
        auto callback = [&](long step) {
            if (step % s.logging_interval == 0) show_progress(step);
            if (step % s.sampling_interval == 0) save_sample();
            if (step % s.loop_update_interval == 0) step_loops(step);
            if (step % s.glue_update_interval == 0) step_glues(step);
        };
        chk(gd_begin_phase(_sys, nullptr));
        for (std::size_t r = 0; r < _replicas.size(); r++) upload_loops(r, -1);
        callback(0);
        std::vector<uint64_t> seeds;      // every trajectory's integrator seed, drawn where simulation draws it
        for (auto &t : _replicas) {
            seeds.push_back(t->random());
            if (t->trace.is_open()) t->trace << "seed " << seeds.back() << '\n' << std::flush;
        }
        gd_run_desc run{};
        run.temperature = s.temperature; run.timestep = s.timestep; run.seed = seeds[0]; run.noise_mode = GD_NOISE_PHILOX;
        run.replica_seeds = seeds.data();
        long step = 0;
        while (step < s.steps) {
            long const next = std::min<long>(s.steps, std::min({next_multiple(step, s.logging_interval), next_multiple(step, s.sampling_interval),
                                                               next_multiple(step, s.loop_update_interval), next_multiple(step, s.glue_update_interval)}));
            run.steps = next - step; chk(gd_run(_sys, &run)); step = next;
            callback(step);
        }
    }

    simulation_config _config;
    std::vector<chain_assignment> _chains;
    std::vector<std::unique_ptr<replica>> _replicas;
    gd_system *_sys = nullptr;
    std::size_t _n = 0;
    gd_bond_params _loop_bond{}, _glue_bond{};
    std::vector<double> _xyz;        // (K, N, 3)
    bool _auto_skin = false;
    bool _device_glues = false;
    std::vector<uint32_t> _glue_counts;      // --device-glues: the set sizes after the last update (gd_glue_counts)
};

// "s0,s1,...": distinct unsigned integers
std::vector<std::uint64_t> parse_seeds(std::string const &text)
{
    std::vector<std::uint64_t> seeds;
    std::size_t pos = 0;
    while (pos <= text.size()) {
        std::size_t const end = std::min(text.find(',', pos), text.size());
        std::string const item = text.substr(pos, end - pos);
        if (item.empty() || item.find_first_not_of("0123456789") != std::string::npos) throw std::runtime_error{"--seeds takes a comma-separated list of unsigned integers"};
        std::uint64_t const seed = std::stoull(item);
        if (std::find(seeds.begin(), seeds.end(), seed) != seeds.end()) throw std::runtime_error{"--seeds: seed " + item + " is listed twice"};
        seeds.push_back(seed);
        pos = end + 1;
    }
    return seeds;
}

void show_usage()
{
    std::cerr << "Loop formation simulator\n"
                 "usage: main [-hCosd] <config>\n\n"
                 "  <config>     JSON file specifying simulation parameters\n\n"
                 "options:\n"
                 "  -C <config>  override chain definitions (config 'chains' key) by additional JSON file\n"
                 "  -o <output>  override output HDF5 filename (config 'output_filename' key)\n"
                 "  -s <seed>    override random seed (config 'random_seed' key)\n"
                 "  --seeds <s0,s1,...> run one trajectory per seed as the replicas of one device handle; the output name\n"
                 "               must contain {seed}; not with -s\n"
                 "  --device-glues  with --seeds: glue binding and unbinding of all trajectories on the device, one call per\n"
                 "               update, with counter-based draws keyed by each seed (deterministic; not the host's mt19937_64\n"
                 "               sequence)\n"
                 "  -d <device>  GPU index (default 0)\n"
                 "  --auto-skin  select the neighbour-list width from measured step times (faster on some models; the\n"
                 "               trajectory of a seed then depends on timing -- off by default)\n"
                 "  --trace <dir> write the initial positions and every uploaded loop / glue list to <dir> (replay support)\n"
                 "  -h           print this usage message and exit\n\n";
}

std::string load_text(std::string const &filename)
{
    std::ifstream file{filename};
    std::string text;
    if (!std::getline(file, text, '\0')) throw std::runtime_error{"failed to load config file"};
    return text;
}

}  // namespace

int main(int argc, char **argv)
{
    try {
        std::optional<std::string> chains_filename, output_filename;
        std::optional<std::uint64_t> seed;
        std::vector<std::string> positional;
        int device = 0;
        std::string trace_dir;
        bool auto_skin = false;
        std::optional<std::vector<std::uint64_t>> seeds;
        bool device_glues = false;
        for (int i = 1; i < argc; i++) {
            std::string const arg = argv[i];
            auto value = [&]() -> std::string { if (i + 1 >= argc) throw std::runtime_error{"bad option"}; return argv[++i]; };
            if (arg == "-h") { show_usage(); return 0; }
            else if (arg == "-C") chains_filename = value();
            else if (arg == "-o") output_filename = value();
            else if (arg == "-s") seed = std::stoull(value());
            else if (arg == "--seeds") seeds = parse_seeds(value());
            else if (arg == "-d") device = std::stoi(value());
            else if (arg == "--trace") trace_dir = value();
            else if (arg == "--device-glues") device_glues = true;
            else if (arg == "--auto-skin") auto_skin = true;
            else if (arg == "--fixed-skin") auto_skin = false;
            else if (arg.size() > 1 && arg[0] == '-') throw std::runtime_error{"bad option"};
            else positional.push_back(arg);
        }
        if (positional.size() != 1) throw std::runtime_error{"config file is not specified"};
        if (device_glues) {      // (refused here: before the configuration is read and before any output or trace file exists)
            if (!seeds) throw std::runtime_error{"--device-glues needs --seeds (one seed or more)"};
            if (!gd_glue_define || !gd_glue_update || !gd_glue_fetch || !gd_glue_counts || !gd_replica_pairs_define || !gd_replica_pairs_set)
                throw std::runtime_error{"--device-glues needs the device glue kinetics (gd_glue_*, gdyn_glue.h), which this gdyn library does not have"};
        }
        simulation_config config;
        {
            auto const text = load_text(positional[0]);
            try {
                config = parse_simulation_config(text);
            } catch (std::exception const &err) {
                throw std::runtime_error{"failed to parse config file - " + std::string{err.what()}};
            }
        }
        if (chains_filename) {
            auto const text = load_text(*chains_filename);
            try {
                config.chains = parse_chains_config(text);
            } catch (std::exception const &err) {
                throw std::runtime_error{"failed to parse chains config file - " + std::string{err.what()}};
            }
        }
        if (output_filename) config.sampling.output_filename = *output_filename;
        if (seeds) {
            if (seed) throw std::runtime_error{"--seeds and -s exclude each other"};
            std::string const &name = config.sampling.output_filename;
            std::size_t const at = name.find("{seed}");
            if (at == std::string::npos) throw std::runtime_error{"--seeds: the output name '" + name + "' must contain {seed}"};
            std::vector<std::string> outputs;
            for (auto s : *seeds) outputs.push_back(std::string{name}.replace(at, 6, std::to_string(s)));
            if (seeds->size() == 1 && !device_glues) { seed = seeds->front(); config.sampling.output_filename = outputs.front(); }      // exactly -s
            else {
                if (!gd_replica_pairs_define || !gd_replica_pairs_set)
                    throw std::runtime_error{"--seeds with several seeds needs per-replica dynamic pair lists (gd_replica_pairs_*, gdyn_replica.h), "
                                             "which this gdyn library does not have"};
                ensemble{config, *seeds, outputs, device, trace_dir, auto_skin, device_glues}.run();
                return 0;
            }
        }
        if (seed) config.sampling.random_seed = *seed;
        simulation{config, device, trace_dir, auto_skin}.run();
        return 0;
    } catch (std::exception const &err) {
        std::cerr << "error: " << err.what() << '\n';
        return 1;
    }
}
