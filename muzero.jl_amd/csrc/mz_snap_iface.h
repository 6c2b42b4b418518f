// mz_snap_iface.h — the engine's internal interface for snapshots
// (mz_snapshot.hip).  Host-side only, not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "mz_ckpt_iface.h"
#include "mz_selfplay_params.h"
#include "mz_snap_layout.h"

// The device state a snapshot holds, as the engine has it right now.
struct MzSnapView {
    int device = 0;
    hipStream_t stream = nullptr;
    int env = -1, G = 0, cap = 0, T = 0, osz = 0, A = 0, per = 0;
    uint64_t seed = 0;
    SpHist ring{}, hist{};                  // ring.rcv null: not allocated
    long long* counters = nullptr;          // [MZ_SP_COUNTERS]
    uint8_t* board = nullptr; int32_t* player = nullptr; uint8_t* over = nullptr;
    uint32_t* ekey = nullptr; float* tgame = nullptr; long long* eval = nullptr;
    int reset_pending = 0;
    // mz_train_init ran: {batch size, learner step t, actor refreshes}, the actors' and the queued flat vectors
    int train = 0;
    long long tr[3] = {0, 0, 0};
    float* actor = nullptr; float* queued = nullptr;
    size_t nflat = 0;
    std::string settings;                   // the handle's settings as JSON (informational)
};

// waits for the device (MZ_SYNC); refused before mz_selfplay_init
int mz_snap_view(mz_handle* h, MzSnapView* v);
void mz_snap_engine_geometry(const mz_handle* h, mzsnap::EngineGeometry* e);
// what mz_selfplay_init(env, G, cap) performs (the handle's mz_selfplay_mode is kept), ring.rcv and
// the reanalyse search's io if `rcv`, the weight sets of mz_train_init if `train`; then the new view
int mz_snap_restore_begin(mz_handle* h, int env, int G, int cap, bool rcv, bool train, MzSnapView* v);
// after the device state is in place: the host's mirrors of it (tr == nullptr: no train section)
int mz_snap_restore_end(mz_handle* h, const long long* counters, int reset_pending, const long long* tr);
