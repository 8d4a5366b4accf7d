// ba_map_graph.h — the pinned rules of ba_map_graph (include/ba_hip.h),
// written once for the device (ba_map_graph.hip) and for host programs
// (host/ba_batch_pack.hpp's restatement, tests/cpp/map_graph_host.cpp): plain
// C++ behind __host__ __device__.  Everything is integers but the culling
// vote, which compares two doubles formed from integers.
#pragma once
#include <stdint.h>

#include "../../include/ba_hip.h"

#if defined(__HIPCC__)
#define BA_MG_HD __host__ __device__
#else
#define BA_MG_HD
#endif

namespace bahip {

// The list is ascending by this key (Frame.cpp:359: sort of pair<weight, frame>)
BA_MG_HD inline uint64_t mg_list_key(int32_t w, int32_t g) { return ((uint64_t)(uint32_t)w << 32) | (uint32_t)g; }
// The fallback is the largest of these: the largest weight, then the lowest index (Frame.cpp:352-357)
BA_MG_HD inline uint64_t mg_fallback_key(int32_t w, int32_t g) { return ((uint64_t)(uint32_t)w << 32) | (0xffffffffu - (uint32_t)g); }
// a comes before b in the list by descending weight, ties in ascending index
BA_MG_HD inline bool mg_stronger(int32_t wa, int32_t ga, int32_t wb, int32_t gb) { return wa > wb || (wa == wb && ga < gb); }

// SfMHelper.cpp:1040-1052: an other view counts when its octave is at most one above the observation's
BA_MG_HD inline bool mg_view_counts(int32_t other_octave, int32_t octave) { return other_octave <= octave + 1; }
constexpr int kMgMinTrack = 3, kMgMinViews = 3;   // a redundant observation: track longer than 3, at least 3 such views

// SfMHelper.cpp:1068: frames 0 and 1 are never culled
BA_MG_HD inline int32_t mg_cull(int32_t frame_id, int32_t n_map, int32_t n_red, double fraction) {
  return frame_id != 0 && frame_id != 1 && (double)n_map * fraction < (double)n_red ? 1 : 0;
}

// cullRecentMapPoints / eraseOutlier (SfMHelper.cpp:974-1017, 1111)
BA_MG_HD inline uint8_t mg_point_status(bool invalid, int64_t age, int32_t track) {
  if (invalid) return BA_GRAPH_PT_INVALID;
  if (age >= 4 && track <= 2) return BA_GRAPH_PT_ERASE;
  if (age >= 5) return BA_GRAPH_PT_MATURE;
  return BA_GRAPH_PT_RECENT;
}

// Column tile of the weight histogram (int32 counters in LDS): 8192 frames are
// 32 KiB, which leaves room for five workgroups on a CU's 160 KiB.
constexpr int kMgTileMax = 8192;
// Device scratch that a chunk of queries may take (W rows, sorted lists, bitmaps)
constexpr size_t kMgChunkBudget = (size_t)256 << 20;
constexpr int kMgThreads = 256;

}  // namespace bahip
