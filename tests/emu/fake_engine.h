// fake_engine.h -- what tests/emu/facade_driver.cpp tells tests/emu/fake_engine.cpp (a stand-in for the engine functions
// the Detector facade links; no GPU, no HIP) beside the C ABI of include/sbm.h itself.
#ifndef SBM_FAKE_ENGINE_H
#define SBM_FAKE_ENGINE_H

#include <string>

// forget everything: log, script, registered buffers; the next sbm_create is context 0
void fake_reset();
// buffers are logged by the name registered for their address (frames, masks, pinned blocks), never by address; a buffer
// nobody registered (the facade's continuous copy of a mask view) is logged as copy:<hash of its bytes>
void fake_register(const void* p, const char* name);
void fake_log_enable(bool on); // off: calls are not logged and new contexts get no ordinal
std::string fake_log();

// the script
void fake_fail_begin(int ctx, int kth, int code, const char* msg); // the kth (0-based) begin on context ctx returns code
void fake_fail_end(int ctx, int code, const char* msg);            // the next end on context ctx returns code
// the frame whose pixels start at p has n records (n < 0: its batch count reads n; INT_MIN: as it comes) and, in a batch,
// its overflow word set
void fake_frame_reports(const void* p, int n, bool overflow);

#endif
