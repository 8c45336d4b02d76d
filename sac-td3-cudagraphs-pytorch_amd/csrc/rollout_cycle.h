// What crosses between engine.hip, env.hip and rollout_cycle.hip for sactd3_rollout_cycle (include/sactd3_rollout_cycle.h): the
// argument struct and the launchers of the graph form of the ring append (rollout_cycle.hip: the only device code of the cycle that is
// new), and the one entry by which the rollout handle (env.hip) asks the engine (engine.hip) for a cycle.  Nothing else crosses: the
// engine never sees the env handle -- it is handed a launcher plus its context -- and the rollout never sees the engine's fields.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

struct sactd3_engine;

// ---- k_rb_ingest_g / k_rb_publish_g (rollout_cycle.hip)
// k_rb_ingest with the cursor taken from device memory: `n` records at `src` go to the slots cursor, cursor + 1, ... (wrapping at `cap`),
// {len, cursor} being the two adjacent device words at `ring_words` (DevCtl::rb_len, rb_cursor) -- a captured graph would freeze a
// launch argument.  Afterwards the words hold len' = min(cap, len + n) and cursor' = (cursor + n) mod cap.
// Read, THEN publish: a block that starts late must not find the new cursor.  publish == 1 (the launch is ONE block): that block
// publishes behind a barrier that every one of its threads reaches after its read.  publish == 0 (several blocks): the launch writes no
// word, and the single-thread k_rb_publish_g behind it -- the next node of the same stream -- does.  No block ever waits for another.
// A length outside [0, cap] or a cursor outside [0, cap) never becomes an address: both are clamped first, and the publishing thread
// counts the append in *clamped (a word of the engine's own, 0 in every run whose words the engine's own launches wrote).
struct IngestArgsG {
  const float4* src; float4* ring; int rec4, n, cap;
  int* ring_words;
  int* clamped;
  int publish;
};
// float4 chunks per block of k_rb_ingest_g; ingest_g_blocks: the grid that gives every chunk of an n-record slab a thread
#define INGEST_G_BLOCK 256
static inline unsigned ingest_g_blocks(long n, int rec4) { return (unsigned)((n * rec4 + INGEST_G_BLOCK - 1) / INGEST_G_BLOCK); }
// One launch each on `stream`.  hipErrorInvalidValue, and nothing is launched, where the host can see that an argument is outside what
// the kernel holds (a NULL pointer, a slab or ring that is not 16-byte aligned, words that are not 8-byte aligned, n outside [1, cap],
// n * rec4 >= 2^31, publish == 1 with more than one block); otherwise
// hipGetLastError() behind the launch.
hipError_t rb_ingest_g_launch(const IngestArgsG& args, unsigned blocks, hipStream_t stream);
hipError_t rb_publish_g_launch(const IngestArgsG& args, hipStream_t stream);

// ---- the cycle (engine.hip), as the rollout handle asks for it (env.hip)
struct CycleBinding {
  const void* owner;                              // the rollout handle: the cycle graphs are its binding's, a cycle of another owner drops them
  int (*env_step)(void* ctx, hipStream_t s);      // the one launch of k_env_step_rec on `s`, every argument fixed for the owner's life; 0 or a hipError_t
  void* ctx;
  float* obs; int64_t obs_ld;                     // the caller's three buffers: by value in the graph's nodes
  float* actions; int64_t actions_ld;
  const float* records;
  int n;                                          // num_envs: the rows of all three
  hipStream_t stream;                             // the rollout's stream, ordered around the cycle once per call
  int64_t* stats;                                 // the owner's {cycles issued, graphs captured, nodes of the last graph launched, cycles issued eagerly}
};
// env step -> append -> acting pair -> uniform iteration on the engine's stream, as one graph launch (use_graphs == 0: the same launches,
// eagerly); `explore`: the acting pair's mode.  -> 0 or a SACTD3_E* code with the text in sactd3_last_error(e); a refused call has changed nothing.
int engine_rollout_cycle(sactd3_engine* e, const CycleBinding& b, int explore, int do_actor);
// the owner goes away (or never cycled: a no-op): its graphs are dropped behind a wait for the engine's stream
void engine_rollout_cycle_release(sactd3_engine* e, const void* owner);
// appends of the cycle whose device words were clamped (IngestArgsG::clamped), read behind a wait for the engine's stream
int engine_rollout_cycle_clamped(sactd3_engine* e, int64_t* out);
