// Stand-alone host check of the arena bookkeeping (cgr-mpnn-3d_amd/csrc/arena_book.hpp), which
// capi.hip consults before every backward / input-gradients call.  No GPU and no HIP library:
//   c++ -std=c++17 -pthread -D__HIP_PLATFORM_AMD__ -I$ROCM_PATH/include -Icgr-mpnn-3d_amd/csrc \
//       -fsanitize=address,undefined tools/arena_book_check.cpp -o arena_book_check
// and once more with -fsanitize=thread.  Exit status 0 and "ok" on success.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>

#include "arena_book.hpp"

using cgr::ArenaBook;
using cgr::OutLevel;

#define EXPECT(cond)                                              \
  do {                                                            \
    if (!(cond)) {                                                \
      fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

constexpr int kTrain = CGR_TRAIN_FOR_BACKWARD;
constexpr int kTrainDrop = CGR_TRAIN_FOR_BACKWARD | CGR_TRAIN_DROPOUT;

static bool is(const ArenaBook::Seen& s, int flags, int mode, OutLevel level, bool here) {
  return s.flags == flags && s.mode == mode && s.level == level && s.backward_here == here;
}

// what capi.hip's forward_entry does around a forward that succeeds
static void forward(ArenaBook& book, const void* arena, int flags, int mode, OutLevel level) {
  book.note_forward(arena, -1);
  book.note_forward(arena, flags, mode, level);
}

// forward -> backward -> input grads -> second forward, on arenas / workspaces of `base`'s own
static void sequences(ArenaBook& book, char* base) {
  const void *a = base, *a2 = base + 1, *ws = base + 2, *ws2 = base + 3;
  EXPECT(is(book.seen(a, ws), -1, -1, OutLevel::Fused, false));  // never seen

  forward(book, a, kTrain, 0, OutLevel::Fused);
  EXPECT(is(book.seen(a, ws), kTrain, 0, OutLevel::Fused, false));  // no backward yet
  book.note_backward(a, ws);
  EXPECT(is(book.seen(a, ws), kTrain, 0, OutLevel::Fused, true));
  EXPECT(is(book.seen(a, ws), kTrain, 0, OutLevel::Fused, true));  // input grads may repeat
  EXPECT(!book.seen(a, ws2).backward_here);                        // another workspace
  EXPECT(!book.seen(a).backward_here);                             // none given
  EXPECT(is(book.seen(a2, ws), -1, -1, OutLevel::Fused, false));   // another arena

  // a second forward makes the workspace stale, from the moment it starts
  book.note_forward(a, -1);
  EXPECT(is(book.seen(a, ws), -1, -1, OutLevel::Fused, false));
  book.note_forward(a, kTrainDrop, 1, OutLevel::Pooled);
  EXPECT(is(book.seen(a, ws), kTrainDrop, 1, OutLevel::Pooled, false));
  book.note_backward(a, ws);
  EXPECT(book.seen(a, ws).backward_here);

  // a wrong-level arena: each level is reported as the one that filled it
  forward(book, a2, kTrain, 0, OutLevel::Nodes);
  EXPECT(book.seen(a2).level == OutLevel::Nodes && book.seen(a).level == OutLevel::Pooled);
  // the workspace taken over by another arena's backward no longer serves the first
  book.note_backward(a2, ws);
  EXPECT(book.seen(a2, ws).backward_here && !book.seen(a, ws).backward_here);

  // a forward that fails, or a predict: only the invalidating note
  book.note_forward(a2, -1);
  EXPECT(is(book.seen(a2, ws), -1, -1, OutLevel::Fused, false));
  // a forward without CGR_TRAIN_FOR_BACKWARD keeps its flags for the message
  forward(book, a2, 0, 0, OutLevel::Fused);
  EXPECT(is(book.seen(a2, ws), 0, 0, OutLevel::Fused, false));
}

int main() {
  ArenaBook book;
  static char mem[3][8];
  // two threads on arenas of their own, and both on one shared arena: a reader must see one
  // moment of it -- the record of forward A, of forward B, or the invalidated one between
  const void *shared = mem[2], *sws = mem[2] + 1;
  std::atomic<bool> stop{false};
  std::thread writer([&] {
    sequences(book, mem[0]);
    for (int i = 0; i < 20000; ++i) {
      forward(book, shared, kTrain, 0, OutLevel::Fused);
      book.note_backward(shared, sws);
      forward(book, shared, kTrainDrop, 1, OutLevel::Nodes);
    }
    stop = true;
  });
  std::thread reader([&] {
    sequences(book, mem[1]);
    long seen_here = 0;
    while (!stop) {
      const ArenaBook::Seen s = book.seen(shared, sws);
      EXPECT(is(s, -1, -1, OutLevel::Fused, false) ||
             is(s, kTrainDrop, 1, OutLevel::Nodes, false) ||
             (s.flags == kTrain && s.mode == 0 && s.level == OutLevel::Fused));
      seen_here += s.backward_here;
    }
    (void)seen_here;
  });
  writer.join();
  reader.join();
  EXPECT(is(book.seen(shared, sws), kTrainDrop, 1, OutLevel::Nodes, false));
  puts("ok");
  return 0;
}
