// tests only: the host build of mpc_local_planner_amd/csrc/mpc_plant.hpp (the per-instance rule of mpc_plant_step*) behind a C entry point, in the layouts of
// include/mpc_plant.h and include/mpc_fleet.h.  No GPU calls.  With -DPLH_MAIN: a stand-alone program that reads cases from a file written by
// tests/_plant_cases.py (write_cases), runs them through the same entry point and writes the outputs to another file (the sanitizer build of
// tests/test_plant_host.py); the file reader is the siblings' (costmap_case_file.hpp: rd, wr).
#include "../../mpc_local_planner_amd/csrc/mpc_plant.hpp"

#include "costmap_case_file.hpp"

// B instances through pl_instance.  dpar: {map_origin x, y, map_resolution, interval, wheelbase, v_min[3], v_max[3], a_max[3], footprint[16][2]}; ipar: {n_footprint,
// n_substeps, drive, map_size_x, map_size_y, block_threshold, unknown_blocks, outside_blocks}; map nullable; the pool: P entries of V vertices, radius nullable;
// self_index [B], vel [B][3], stall [B] and info [B][4] nullable.  Returns rule 5's Rc (1 without a map or a footprint), -1 when an edge is above the cap (nothing is
// written then).
extern "C" int plh_step(int B, const double* dpar, const int32_t* ipar, const uint8_t* map, const double* cmd, int P, int V, const int32_t* pool_n_vertices,
                        const double* pool_vertices, const double* pool_radius, const int32_t* self_index, double* pose, double* vel, int32_t* stall, int32_t* info) {
    mpc::PlantParams p = {};
    p.map_ox = dpar[0]; p.map_oy = dpar[1]; p.res = dpar[2]; p.dt = dpar[3]; p.wheelbase = dpar[4];
    for (int i = 0; i < 3; ++i) { p.v_min[i] = dpar[5 + i]; p.v_max[i] = dpar[8 + i]; p.a_max[i] = dpar[11 + i]; }
    p.nf = ipar[0]; p.n_sub = ipar[1]; p.drive = ipar[2]; p.map_sx = ipar[3]; p.map_sy = ipar[4]; p.threshold = ipar[5]; p.unknown_blocks = ipar[6] ? 1 : 0;
    p.outside_blocks = ipar[7] ? 1 : 0; p.has_map = map ? 1 : 0;
    for (int j = 0; j < p.nf; ++j) { p.fx[j] = dpar[14 + 2 * j]; p.fy[j] = dpar[15 + 2 * j]; }
    if (!mpc::pl_reach(p)) return -1;
    const mpc::FleetPool pool = {P, pool_n_vertices, pool_vertices, pool_radius, nullptr};
    for (int b = 0; b < B; ++b)
        mpc::pl_instance(p, map, pool, V, self_index ? self_index[b] : -1, cmd + 3 * (size_t)b, pose + 3 * (size_t)b, vel ? vel + 3 * (size_t)b : nullptr,
                         stall ? stall + b : nullptr, info ? info + 4 * (size_t)b : nullptr);
    return p.Rc;
}

extern "C" int plh_list_cap() { return mpc::kPlListCap; }
extern "C" int plh_threads() { return mpc::kPlThreads; }
// the kernel's culling test for one pool entry and one instance (valid instances only): 1 when the entry is kept, 0 when it is dropped, -1 for an invalid instance
extern "C" int plh_kept(const double* dpar, const int32_t* ipar, const double* cmd, const double* pose, const double* vel, int P, int V, const int32_t* pool_n_vertices,
                        const double* pool_vertices, const double* pool_radius, int self, int entry) {
    mpc::PlantParams p = {};
    p.dt = dpar[3]; p.wheelbase = dpar[4];
    for (int i = 0; i < 3; ++i) { p.v_min[i] = dpar[5 + i]; p.v_max[i] = dpar[8 + i]; p.a_max[i] = dpar[11 + i]; }
    p.nf = ipar[0]; p.n_sub = ipar[1]; p.drive = ipar[2];
    for (int j = 0; j < p.nf; ++j) { p.fx[j] = dpar[14 + 2 * j]; p.fy[j] = dpar[15 + 2 * j]; }
    mpc::pl_reach(p);
    mpc::PlantState st;
    double target[3];
    const double none[3] = {0.0, 0.0, 0.0};
    if (!mpc::pl_start(p, pose, cmd, vel ? vel : none, vel != nullptr, st, target)) return -1;
    const mpc::FleetPool pool = {P, pool_n_vertices, pool_vertices, pool_radius, nullptr};
    return mpc::sc_may_reach(pool, V, entry, self, st.x, st.y, mpc::pl_cull_radius(p, st, target)) ? 1 : 0;
}

#ifdef PLH_MAIN
// A case in the file: int32 {B, P, V, has_map, has_radius, has_self, has_vel, has_stall, has_info, then ipar}, double dpar, [the map], cmd, pose, [vel], [pool
// n_vertices, vertices, [radius]], [self_index].  Its outputs in the other file: pose, [vel], [stall], [info].
int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s cases outputs\n", argv[0]); return 2; }
    FILE* in = std::fopen(argv[1], "rb");
    FILE* out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::printf("cannot open the files\n"); return 2; }
    int cases = 0;
    std::vector<int32_t> head;
    while (rd(in, head, 17)) {
        const size_t B = head[0], P = head[1], V = head[2];
        const int32_t* ipar = head.data() + 9;
        std::vector<double> par, cmd, pose, vel, pv, pr;
        std::vector<uint8_t> map;
        std::vector<int32_t> pnv, self, stall(head[7] ? B : 0, -7), info(head[8] ? 4 * B : 0, -7);
        if (!(rd(in, par, 46) && rd(in, map, head[3] ? (size_t)ipar[3] * ipar[4] : 0) && rd(in, cmd, 3 * B) && rd(in, pose, 3 * B) && rd(in, vel, head[6] ? 3 * B : 0) &&
              rd(in, pnv, P) && rd(in, pv, P * V * 2) && rd(in, pr, head[4] ? P : 0) && rd(in, self, head[5] ? B : 0))) { std::printf("case %d: short read\n", cases); return 2; }
        if (plh_step((int)B, par.data(), ipar, head[3] ? map.data() : nullptr, cmd.data(), (int)P, (int)V, pnv.data(), pv.data(), head[4] ? pr.data() : nullptr,
                     head[5] ? self.data() : nullptr, pose.data(), head[6] ? vel.data() : nullptr, head[7] ? stall.data() : nullptr, head[8] ? info.data() : nullptr) < 0) {
            std::printf("case %d: refused\n", cases);
            return 2;
        }
        if (!(wr(out, pose) && wr(out, vel) && wr(out, stall) && wr(out, info))) { std::printf("case %d: short write\n", cases); return 2; }
        ++cases;
    }
    std::fclose(in);
    std::fclose(out);
    std::printf("plant_host: %d cases\n", cases);
    return 0;
}
#endif
