// goal_attain.h — goal-attainment selection over a scored grid: per goal / weight vector the candidates
// that minimise gamma = max_j (F_j - goal_j) / w_j, with w_j = 0 a hard constraint
// (mpct_goal_attain_device / mpct_goal_attain, include/mpct.h).  Kernels in goal_attain.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr long long kGoalMaxG = 1 << 20;  // MPCT_GOAL_MAX_G
constexpr int kGoalMaxBest = 16;          // MPCT_GOAL_MAX_BEST
constexpr int kGoalBlock = 256;           // threads of a workgroup: one goal vector g per lane
constexpr int kGoalTile = 256;            // T: candidates per LDS tile [K][T]
constexpr int kGoalTargetBlocks = 2048;   // the candidate range is split until the grid holds about this many workgroups
constexpr int kGoalMaxSplit = 1024;       // chunks of the candidate range at most

struct GoalOut {
  int* best;        // [G][n_best]
  double* gamma;    // [G][n_best]
  int* active;      // [G][n_best]
  int* n_feasible;  // [G]
  int* n_attained;  // [G]
  int* wins;        // [C]
};

// chunks of the candidate range (grid.y) and candidates per chunk (a multiple of the tile) for G goal vectors
// and C candidates; split_override > 0 forces the requested number of chunks (some may then be empty)
void goal_grid(long long G, long long C, int tile, int split_override, int* split, int* chunk);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked.
// tile 0 / split 0: the defaults (kGoalTile, goal_grid); others are the test hook's
int goal_attain_device(const double* costs, long long C, int k, const double* goals, const double* weights, long long G,
                       int n_best, const GoalOut& out, hipStream_t stream, std::string* err, int tile = 0, int split = 0);

}  // namespace mpct
