// uvol_ws.hpp — lifetime-shared device workspaces (host side).  An array is described by its size and the first / last pipeline
// phase that touches it; arrays whose lifetimes do not overlap share addresses (greedy first-fit over the live intervals, largest
// first).  Arrays that must start out zero carry phase UVOL_WS_PINNED: they form the head of the workspace (never shared), which
// one clear kernel zeroes per batch.  Used by the geometry encoder (geom_encode.hip) and the geometry decoder (geom_decode.hip).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

// bytes a device buffer is allocated with when `bytes` are asked for (uvol_ensure): slack against re-allocation for slightly larger
// batches; bounded: an eighth of a 100 GB workspace is frames that could be in flight
static inline size_t uvol_ws_alloc_size(size_t bytes) { return bytes + std::min<size_t>(bytes / 8, (size_t)256 << 20) + 4096; }
// Would every lane of a ring hold a workspace of `ws` bytes?  caps[k] = what lane k holds now (0: nothing yet, or a lane not created).
// A lane that is too small gives its buffer back before it allocates uvol_ws_alloc_size(ws) (uvol_ensure), so the ring grows by the
// differences; that growth has to fit in `free_b` with a sixteenth of the device (`total_b` / 16: 18 GB of 288) to spare.  A ring that
// is large enough already fits whatever is free: nothing is allocated.
static inline bool uvol_ws_ring_fits(size_t ws, const std::vector<size_t> &caps, size_t free_b, size_t total_b) {
  const size_t want = uvol_ws_alloc_size(ws);
  size_t grow = 0;
  for (size_t c : caps) if (c < ws) grow += want - c;
  return grow == 0 || grow + total_b / 16 <= free_b;
}

// Hardware queues the process's streams are spread over: the runtime maps every stream to one of GPU_MAX_HW_QUEUES queues (4 unless the
// variable says otherwise) and streams that share a queue run one after the other, so the geometry ring is shaped for that many
// (uvol_ring_shape below).  The value is READ, never set: `own` = UVOL_HW_QUEUES (tests / diagnostic: changes the library's plan only,
// never the runtime), `rt` = GPU_MAX_HW_QUEUES, both as the environment holds them (nullptr: unset).  Leading digits count, as the
// runtime reads them; no digit at all gives the runtime's default of 4; the result lies in 1..32.
static inline int uvol_hw_queues_from(const char *own, const char *rt) {
  for (const char *s : { own, rt }) {
    if (!s) continue;
    while (*s == ' ' || *s == '\t') s++;
    if (*s == '+') s++;
    if (*s < '0' || *s > '9') continue;
    long v = 0; for (; *s >= '0' && *s <= '9' && v < 1000; s++) v = v * 10 + (*s - '0');
    return (int)std::max<long>(1, std::min<long>(32, v));
  }
  return 4;
}
static inline int uvol_hw_queues() { static const int v = uvol_hw_queues_from(getenv("UVOL_HW_QUEUES"), getenv("GPU_MAX_HW_QUEUES")); return v; }

// Shape of the geometry ring for a queue budget: lanes (one main stream each), groups an enqueued call is cut into, and whether the
// valence replays run on ONE auxiliary stream per context (shared) or one per lane.  lanes_forced / groups_forced: UVOL_GEO_LANES /
// UVOL_GEO_GROUPS (0 = not set), aux_forced: UVOL_GEO_AUX (-1 = not set, 0 = lane, 1 = shared).
//  - A main and an auxiliary stream per lane fit beside one queue for the rest of the process (13 queues or more for six lanes): round
//    5's shape, 6 lanes x 4 groups.
//  - Otherwise the ring stays INSIDE the budget - main streams + 1 <= queues - so that no two main streams have to share a queue (two
//    lanes on one queue run one after the other: a lane then waits for the whole group of its neighbour before its own starts, and the
//    front-end chain passes the wait on): the replays of all lanes run on one shared stream (42 ms of work per 640-frame group against
//    a group every 180 ms), created BEHIND the main streams (geom_encode.hip: geo_shared_aux), and a call is cut into two thirds as many
//    groups as the ring has lanes: the serial chain is flat in the group size, so fewer, larger groups hold the same
//    1.5 calls' worth of frames in the same bytes (3 lanes x 2 groups of 1280 frames for 6 x 4 of 640).
//  - At most THREE lanes on a short budget: 3 x 2 is what was measured (on 4 queues, the runtime's default: 3312 - 3492 frames/s against
//    2847 - 2857 of 6 x 4 with a stream per lane; 4 lanes x 3 groups with the shared stream, five streams on four queues: 2627).
//    Budgets of 5 to 12 queues have not been measured and get the same ring, which fits them too; more lanes there are DESIGN
//    section 7's business.  profiles/r10_queue_budget.json.
// Whether the streams really land on queues of their own is the runtime's placement, which the library can only suggest by the order
// in which it creates them; tools/queue_budget.py on a kernel trace shows it.
// A forced lane count is taken as it is (with round 5's four groups per call unless those are forced too); its auxiliary stream is the
// shared one where that makes the ring fit a short budget, else one per lane as before.
constexpr int UVOL_RING_LANES = 6, UVOL_RING_GROUPS = 4, UVOL_RING_LANES_SHORT = 3, UVOL_RING_LANES_MAX = 16;
struct UvolRingShape { int lanes, groups; bool shared_aux; };
static inline UvolRingShape uvol_ring_shape(int queues, int lanes_forced, int groups_forced, int aux_forced) {
  const int q = std::max(1, std::min(32, queues));
  UvolRingShape s;
  s.lanes = lanes_forced > 0 ? std::min(lanes_forced, UVOL_RING_LANES_MAX) : UVOL_RING_LANES;
  const bool roomy = 2 * s.lanes + 1 <= q;
  if (lanes_forced <= 0 && !roomy) s.lanes = std::max(1, std::min(UVOL_RING_LANES_SHORT, q - 1));
  s.shared_aux = aux_forced >= 0 ? aux_forced == 1 : (!roomy && s.lanes + 1 <= q);
  s.groups = groups_forced > 0 ? groups_forced : ((roomy || lanes_forced > 0) ? UVOL_RING_GROUPS : (2 * s.lanes + 2) / 3);
  return s;
}

#define UVOL_WS_PINNED (-1)
struct UvolWsItem { size_t bytes; int first, last; size_t off; };
// -> offsets in items[].off; returns the total size, *zero = size of the zero-initialised head
static inline size_t uvol_ws_place(std::vector<UvolWsItem> &items, size_t *zero, int n_phases, const char *what) {
  auto a256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
  size_t off = 0;
  for (auto &it : items) if (it.first == UVOL_WS_PINNED) { it.off = off; off = a256(off + it.bytes); }
  *zero = off;
  std::vector<size_t> order;
  for (size_t i = 0; i < items.size(); i++) if (items[i].first != UVOL_WS_PINNED) order.push_back(i);
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return items[a].bytes > items[b].bytes; });
  std::vector<size_t> placed; std::vector<std::pair<size_t, size_t>> busy;
  size_t total = off;
  for (size_t i : order) {
    UvolWsItem &it = items[i];
    busy.clear();
    for (size_t j : placed) if (items[j].first <= it.last && it.first <= items[j].last) busy.emplace_back(items[j].off, a256(items[j].off + items[j].bytes));
    std::sort(busy.begin(), busy.end());
    size_t cur = *zero;
    for (auto &b : busy) { if (cur + it.bytes <= b.first) break; cur = std::max(cur, b.second); }
    it.off = cur; total = std::max(total, a256(cur + it.bytes));
    placed.push_back(i);
  }
  static const bool dump = [] { const char *e = getenv("UVOL_WS_DUMP"); return e && *e == '1'; }();
  if (dump) {
    fprintf(stderr, "[uvol-ws] %s: zero head %.2f MB, total %.2f MB\n", what, *zero / 1e6, total / 1e6);
    for (int ph = 0; ph < n_phases; ph++) { size_t live = 0; for (auto &it : items) if (it.first != UVOL_WS_PINNED && it.first <= ph && ph <= it.last) live += a256(it.bytes); fprintf(stderr, "[uvol-ws]   phase %2d: %.2f MB live\n", ph, live / 1e6); }
  }
  return total;
}
