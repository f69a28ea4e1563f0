// Host-side record of what the last forward left in each arena (capi.hip), kept on the host so
// that a check costs no device sync and holds under graph capture.  Keys are arena addresses; the
// caching allocator reuses them, so the table stays as small as the set of live arena blocks.
// Nothing here touches the GPU.
#pragma once

#include <stdint.h>

#include <mutex>
#include <unordered_map>
#include <utility>

#include "gnn_internal.hpp"  // OutLevel

namespace cgr {

class ArenaBook {
 public:
  // What an entry point needs to know of (arena, workspace), read under one lock: one moment.
  struct Seen {
    // `training` bits of the forward that last filled the arena, -1 if none succeeded: the
    // backward needs the W^T images that only a CGR_TRAIN_FOR_BACKWARD forward packs
    int flags = -1;
    // the precision mode it ran in (enum cgr_precision): the arena's images, counters and saved
    // activations are laid out and filled for that mode, so the backward and the input gradients
    // must be given a config of the same mode
    int mode = -1;
    // its output level (gnn_internal.hpp: the fused y of cgr_gnn_forward, the pooled g of
    // cgr_gnn_encode, the nodes of cgr_gnn_encode_nodes; below the fused level the
    // readout-backward image is unscaled for every pooling mode, and the nodes level leaves the
    // pooling state unwritten): every backward / input-gradients entry refuses an arena of
    // another level
    OutLevel level = OutLevel::Fused;
    // `workspace` holds a backward of the arena's latest forward (below)
    bool backward_here = false;
  };

  // Every forward into an arena starts a new generation of it; flags -1 (before a forward runs,
  // and for a predict) leaves it unusable by a backward.
  void note_forward(const void* arena, int flags, int mode = -1,
                    OutLevel level = OutLevel::Fused) {
    std::lock_guard<std::mutex> lk(mu_);
    Record& r = arenas_[arena];
    r.flags = flags;
    r.mode = mode;
    r.level = level;
    ++r.gen;
  }
  // A backward enqueued on (arena, generation) records its workspace; cgr_gnn_input_grads --
  // which reads dpre0 and the readout's operands from that workspace -- requires the record to
  // name the same arena at its current generation (otherwise it silently returned garbage).
  void note_backward(const void* arena, const void* workspace) {
    std::lock_guard<std::mutex> lk(mu_);
    backward_[workspace] = {arena, arenas_[arena].gen};
  }
  Seen seen(const void* arena, const void* workspace = nullptr) const {
    std::lock_guard<std::mutex> lk(mu_);
    Seen s;
    const auto a = arenas_.find(arena);
    if (a == arenas_.end()) return s;
    s.flags = a->second.flags;
    s.mode = a->second.mode;
    s.level = a->second.level;
    const auto w = backward_.find(workspace);
    s.backward_here = w != backward_.end() && w->second.first == arena &&
                      w->second.second == a->second.gen;
    return s;
  }

 private:
  struct Record {
    int flags = -1, mode = -1;
    OutLevel level = OutLevel::Fused;
    uint64_t gen = 0;
  };
  mutable std::mutex mu_;
  std::unordered_map<const void*, Record> arenas_;
  std::unordered_map<const void*, std::pair<const void*, uint64_t>> backward_;
};

}  // namespace cgr
