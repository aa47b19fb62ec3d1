// mapf_env_large.h -- internal interface between the C ABI in mapf_env.hip and the large-map kernels in mapf_env_large.hip
// (map side 65..128: a map row is two 64-bit words).  Not installed, not part of include/mapf_env.h.
//
// Data layout in HBM of a large handle (the caller-visible layouts of include/mapf_env.h do not change):
//   map_rows Row[E][L]             Row = {uint64_t lo, hi}: bit y of row x = obstacle at (x, y), y < 64 in lo, y >= 64 in hi
//   navi     Row[E][N][L][4]       per (agent, row) one 64-byte record {up, down, left, right} (meaning as for L <= 64)
// Every launcher enqueues on `s` and returns the launch status (hipGetLastError()).
#ifndef MAPF_ENV_LARGE_H
#define MAPF_ENV_LARGE_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mapf_large {

constexpr int kMinLen = 65, kMaxLen = 128;
constexpr size_t kRowBytes = 16;  // one map row; a navigation record is 4 of them

// sticky device status bits: the same values as mapf_env.hip's kStatus* (mapf_check_status decodes them)
constexpr int kStatusAction = 1, kStatusOverlap = 2, kStatusRange = 4, kStatusStage = 8;

struct StepArgs {
    int E, L, N;
    const void *map_rows;
    int16_t *agents;
    const int16_t *goals;
    const void *navi;
    int32_t *steps;
    int32_t *status;
    const int8_t *actions;  // nullptr: observe only
    uint8_t *obs;
    uint32_t *obs_bits;
    int obs_bits_rd;
    int16_t *pos_out;
    int8_t *rclass;
    float *reward;
    uint8_t *done;
    const uint8_t *mask;  // observe only (optional): environments to rewrite
    float rtab[5];
};

hipError_t step(const StepArgs &a, hipStream_t s);
hipError_t pack_maps(int E, int L, const int8_t *maps, void *rows, hipStream_t s);
hipError_t unpack_maps(int E, int L, const void *rows, int8_t *maps, hipStream_t s);
hipError_t scatter_load(int n, int L, int N, const int32_t *ids, const int8_t *maps, const int16_t *agents, const int16_t *goals,
                        void *rows, int16_t *dst_agents, int16_t *dst_goals, int32_t *steps, int E, int32_t *status, hipStream_t s);
// the N fields of every environment (env_ids: of the E listed ones of the handle's E_handle only; env_mask: of the flagged ones only)
hipError_t build_navi(int E, int E_handle, int L, int N, const void *rows, const int16_t *goals, void *navi, int32_t *status,
                      const int32_t *env_ids, const uint8_t *env_mask, hipStream_t s);
hipError_t unpack_navi(long long fields, int L, const void *navi, uint8_t *out, hipStream_t s);
// mapf_reset_envs, direct path: placement + navigation fields of the flagged environments (mask nullptr: all)
hipError_t reset(int E, int L, int N, const uint8_t *mask, float density, uint64_t seed, void *rows, int16_t *agents, int16_t *goals,
                 void *navi, int32_t *steps, int32_t *epochs, int32_t *status, hipStream_t s);
// mapf_stage_next: the next epoch's scenario into the staging arrays of every environment that has none
hipError_t stage_fill(int E, int L, int N, float density, uint64_t seed, void *st_rows, int16_t *st_agents, int16_t *st_goals,
                      void *st_navi, const int32_t *epochs, int32_t *status, int32_t *st_epoch, uint8_t *st_need, hipStream_t s);
// mapf_reset_envs, staged path: the flagged environments take their staged scenario over
hipError_t stage_swap(int E, int L, int N, const uint8_t *mask, void *rows, int16_t *agents, int16_t *goals, void *navi, int32_t *steps,
                      int32_t *epochs, int32_t *status, const void *st_rows, const int16_t *st_agents, const int16_t *st_goals,
                      const void *st_navi, const int32_t *st_epoch, hipStream_t s);

}  // namespace mapf_large

#endif  // MAPF_ENV_LARGE_H
