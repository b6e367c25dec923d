// What a stand-alone harness that builds a bare wn_ctx has to supply in place of wn_api.hip and the per-path translation units: the allocator
// seam of csrc/wn_dev.h (plain runtime calls, no counters) and the deleters of the per-path states a bare context never creates.  The deleters are
// EMPTY: a harness that did create a Synth / SynthF32 / Pipe / F32State would leak it -- such a harness links the state's translation unit instead.
// Non-inline definitions: include this from ONE translation unit of the tool.
#pragma once
#include "wn_common.h"
hipError_t wn_dev_alloc(void** p, size_t bytes, bool pinned) { return pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes); }
void wn_dev_free(void* p, bool pinned) { (void)(pinned ? hipHostFree(p) : hipFree(p)); }
void WnStateDelete::operator()(Synth*) const {}
void WnStateDelete::operator()(SynthF32*) const {}
void WnStateDelete::operator()(Pipe*) const {}
void WnStateDelete::operator()(F32State*) const {}
