// step_parts.h — how a plan runs one PART of its step (the graph part on a side stream, the layers part on the caller's):
// eagerly the first time, captured as a hipGraph the second, replayed from then on.  Written once for the training plans
// (pipeline.hip) and the typed inference plan (hgt_plan.hip); the capture itself (gigl_capture) also serves the one-call
// plan's segments (pipeline.hip capture_segments).  Internal, nothing exported.
#pragma once

#include "common.h"

#include <cstdio>

namespace {

// one part's captured graph, per workspace
struct PartGraph {
  hipGraphExec_t exec = nullptr;
  bool warm = false;  // one eager run of the part has sized arenas / built tables / set kernel attributes
  void drop() {       // (the caller has synchronised the stream it was captured on; `warm` stays)
    if (exec) hipGraphExecDestroy(exec);
    exec = nullptr;
  }
};

// capture the launches `body` issues on `st` and instantiate them as *exec.  body's own failure is returned as it is; HIP's
// is reported on `report` as "capturing <what> failed" (*exec stays null)
template <typename Body>
int32_t gigl_capture(gigl_ctx* report, hipStream_t st, const char* what, hipGraphExec_t* exec, Body&& body) {
  hipGraph_t graph = nullptr;
  int32_t rc = GIGL_OK;
  hipError_t err = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (err == hipSuccess) {
    rc = body();
    const hipError_t e2 = hipStreamEndCapture(st, &graph);
    if (rc == GIGL_OK && e2 != hipSuccess) err = e2;
  }
  if (rc == GIGL_OK && err == hipSuccess) err = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
  if (graph) hipGraphDestroy(graph);
  if (rc != GIGL_OK) return rc;
  if (err != hipSuccess) {
    *exec = nullptr;
    return gigl_fail(report, GIGL_E_HIP, "capturing %s failed: %s", what, hipGetErrorString(err));
  }
  return GIGL_OK;
}

// run `body` on sc->stream: eagerly the first time (arena sizing, table builds and kernel attributes cannot happen inside
// a capture), captured the second, replayed from then on.  capture_ok == false (an A/B knob, timers, an odd batch size) or
// the legacy default stream (it cannot be captured): eagerly, every time.  HIP's failures are reported on `report`;
// `what` names the step in the message of a failed capture
template <typename Body>
int32_t gigl_run_part(gigl_ctx* report, gigl_ctx* sc, PartGraph* g, bool capture_ok, const char* what, Body&& body) {
  hipStream_t st = sc->stream;
  if (!capture_ok || st == nullptr) return body();
  if (!g->exec && !g->warm) {
    const int32_t rc = body();
    if (rc != GIGL_OK) return rc;
    GIGL_HIP_CHECK(report, hipStreamSynchronize(st));
    g->warm = true;
    return GIGL_OK;
  }
  if (!g->exec) {
    char part[96];
    snprintf(part, sizeof part, "a part of the %s", what);
    const int32_t rc = gigl_capture(report, st, part, &g->exec, body);
    if (rc != GIGL_OK) return rc;
  }
  GIGL_HIP_CHECK(report, hipGraphLaunch(g->exec, st));
  return GIGL_OK;
}

}  // namespace
