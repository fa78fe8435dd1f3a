// Clip capture (fvad_engine_enable_capture; DESIGN.md section 7, "Clip
// capture"): argument blocks and launchers of the kernels in
// fvad_capture.hip.
//
//   history ring  [s][c][H] f32: every input sample of the last `history`
//                 samples of each stream, written by k_hist_append on the
//                 stream that reads the push's device input; or, for a capture
//                 of the denoised rows, every denoised sample at the clip
//                 rate, written by k_den_append on the engine stream
//   capture pass  behind a push's machine pass on the side stream: k_cap_plan
//                 (pending queues, due clips, pool offsets), k_cap_channel
//                 (the lowest-RMS channel of each due clip), k_cap_copy (ring
//                 to the pinned pool), k_cap_publish (descriptors and header
//                 to pinned memory)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "fvad_capture_core.h"
#include "fvad_lifecycle.h"
#include "fvad_staged.h"

namespace fvad {

// A stream's place in its history: it holds `pos` samples of this life, which
// began at sample `base`; `wpos` counts every sample the slot ever appended and
// never goes back, so sample n (pos - history <= n < pos) sits at ring index
// (wpos - (pos - n)) % H.  A reset or restore moves pos and base, not wpos: the
// words a capture pass may still be reading are never the next append's.
struct CapPos {
  unsigned long long pos, base, wpos, pad;
};
struct CapWork {  // one due clip of a pass, in delivery order
  int stream;
  unsigned seq;
  int channel;  // written by k_cap_channel; -1: no audio
  unsigned flags;
  unsigned long long from, to, first, n;
  unsigned long long widx;      // ring index of sample `first`
  unsigned long long pool_off;  // pool cursor of the clip's first sample
};
struct CapClip {  // fvad_clip (include/fvad.h), 64 bytes
  int stream;
  unsigned seq;
  int channel;
  unsigned flags;
  unsigned long long push, sample_from, sample_to, first_sample, n_samples, reserved;
};
struct CapHeader {  // what a finished pass tells the host
  unsigned long long pass, desc_end, pool_end, lost;
};
struct CapState {  // device: the cursors, and the running pass's work list size
  unsigned long long desc_wr, pool_wr, lost;
  unsigned long long desc_wr0;  // desc_wr before the running pass
  unsigned n_work, pad;
};

struct CapAppendArgs {
  const float *pcm;          // [t][s][c][480]
  const int16_t *pcm16;      // nullable: the same as 16-bit samples k (k / 32768)
  const int *ticks_valid;    // nullable
  int n_ticks, n_streams, n_channels;
  float *hist;               // [s][c][H]
  unsigned long long H;
  CapPos *pos;               // [s], owned by the appending stream
  CapPos *snap;              // [s] the positions after this push, for its capture pass
  // a capture of the denoised rows (FVAD_CLIP_SOURCE_DENOISED): den set, pcm
  // and pcm16 null, and everything above counts samples of the clip rate
  const float *den;          // nullable: [t][s][c][frame], d_den or the output resampler's rows
  int frame;                 // samples of a tick and channel: 480, or the clip rate / 100
};

struct CapPassArgs {
  const VadmEvRec *stage;    // the machine pass's staged events [lane][ev_cap]
  const unsigned *count;     // [lane]
  int ev_cap, n_machines, machine, n_streams, n_channels;
  int flush_mode;            // 0: a push's pass; 1: flush the streams flagged in `flush`; 2: flush all
  const unsigned char *flush;  // [s] (flush_mode 1)
  const CapPos *pos;         // [s] the push's snapshot (the live positions for a flush)
  cap::Pend *pend;           // [s][cap::kQueue]
  unsigned *pend_n;          // [s]
  unsigned long long history, H;
  const float *hist;
  CapState *state;
  CapWork *work;             // [cap::kQueue * n_streams]
  float *pool;               // pinned, [pool_cap]
  unsigned long long pool_cap;
  CapClip *desc;             // pinned, [desc_cap]
  unsigned long long desc_cap;
  CapHeader *header;         // pinned
  unsigned long long pass, push;
  unsigned long long host_desc_read, host_pool_read;  // the host's read cursors when the pass was enqueued
  // The clip rate 48000 L / M (1, 1 for the 48 kHz signals): pos, history, H
  // and a clip's first / n count its samples, a segment's bounds go through
  // cap::to_rate.  pool16: the pool of an s16 capture (pool is null then).
  unsigned L, M;
  int16_t *pool16;           // pinned, [pool_cap]
  unsigned long long reserved;  // fvad_clip.reserved of every descriptor
};

struct CapSetArgs {  // the listed streams' position and base to value[i]; their pending clips dropped
  CapPos *pos;
  unsigned *pend_n;
  IdList ids;
  unsigned long long value[kListMax];
};

// k_hist_append, then k_hist_advance, on the input's reading stream
hipError_t launch_hist_append(const CapAppendArgs &a, hipStream_t stream);
// the four kernels of one pass, in order on `stream`
hipError_t launch_capture_pass(const CapPassArgs &a, hipStream_t stream);
// the positions of the listed streams (on the appending stream) / their pending queues (on the side stream)
hipError_t launch_capture_set_pos(const CapSetArgs &a, hipStream_t stream);
hipError_t launch_capture_drop(const CapSetArgs &a, hipStream_t stream);

}  // namespace fvad
