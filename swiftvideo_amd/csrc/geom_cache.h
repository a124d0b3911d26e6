// geom_cache.h — tables of the strip kernels' per-layer geometry: their layout, what a batch owns, the device's store (geom_store.cpp; device
// side: wave_common.hip.h).
//
// WaveStrip::setup (wave_common.hip.h) derives, per layer and strip, the column entries (per lane), the row table (LDS) and the staging
// rectangles from nothing but the layer's three matrices, the source planes' sizes, the canvas size, the strip's position and the launch's LDS
// layout — ~230 vector + ~300 scalar instructions, 30 % of the launch on the strip kernels' one- and two-layer ticks
// (profiles/r06_notes.md section 9).  In a batch the same (layer geometry, strip) pair recurs in every tick: the values are computed ONCE per
// batch and launch configuration by a small kernel that runs that very code (same inputs, same instructions, same bits), stored factored into
// one record per strip COLUMN and one per strip ROW (they are functions of the column / of the row alone; what mixes both — staged or not,
// inside or not, rectangle at a picture edge or not — is a flag word per strip), and the tick kernels load them.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "device_types.h"
#include "tick_route.h"

// 1: layers of a batch take their per-strip geometry from the batch's tables (WaveStrip::setup_cached); 0: always computed in place
#ifndef CHV_GEOM_CACHE
#define CHV_GEOM_CACHE 1
#endif

namespace chv {

// (WTW, the strip width: tick_route.h)

// ---- a table's layout (one per geometry class: same matrices, source plane sizes, canvas size) ----------------------------------------------
// [GeomHdr][flag word per strip, row-major, padded to 16 bytes][GeomCol per strip column][row record (row_bytes) per strip row].  The host lays
// it out and writes the header (geom_store.cpp); geom_precompute fills the rest; the kernels find the parts through the header's offsets.
struct GeomHdr { int32_t strips_x, strips_y, wth, row_bytes; uint32_t flags_off, cols_off, rows_off, pad; };     // at the table's base
static_assert(sizeof(GeomHdr) == 32 && offsetof(GeomHdr, row_bytes) == 12 && offsetof(GeomHdr, flags_off) == 16 && offsetof(GeomHdr, cols_off) == 20 &&
              offsetof(GeomHdr, rows_off) == 24, "WaveStrip::setup_cached / geom_store read the header at these offsets");
// a strip column (GeomCol, wave_common.hip.h): uint4 a[64], uint4 b[64], int32_t s[16]
constexpr size_t kGeomColBytes = 2 * WTW * 16 + 16 * 4;
// one class for geom_precompute: a representative layer (its plane POINTERS are not used), the canvas, the table
struct GeomJob {
    DLayer layer;
    int32_t W, H, strips_x, strips_y, first_block, pad;
    uint8_t *table;
};
static_assert(offsetof(GeomJob, W) == sizeof(DLayer) && offsetof(GeomJob, first_block) == sizeof(DLayer) + 16 && offsetof(GeomJob, table) == sizeof(DLayer) + 24 &&
              sizeof(GeomJob) == sizeof(DLayer) + 32, "geom_precompute reads the job list with this layout");
// the table address a DLayer carries in pad2 (0: none)
inline void geom_set_table(DLayer &L, const void *table) {
    const uint64_t tp = (uint64_t)(uintptr_t)table;
    L.pad2[0] = (int32_t)(uint32_t)(tp & 0xFFFFFFFFu); L.pad2[1] = (int32_t)(uint32_t)(tp >> 32);
}
inline void *geom_table(const DLayer &L) { return (void *)(uintptr_t)(((uint64_t)(uint32_t)L.pad2[1] << 32) | (uint64_t)(uint32_t)L.pad2[0]); }

// (GeomConfig, what the tables were built for, and wave_geom_config, which answers it for a launch: tick_route.h)

// The tables of one launch's layers, handed to the strip kernels' launcher (launch_tick_fast -> launch_wave_layers): a batch's (chv_batch), the
// temporary one of a lone tick that builds, or the answer the store gave a lone tick before its layers travelled (built + patched, no layer arrays).
struct GeomCache {
    bool built = false;          // tables hold `config`'s geometry and the batch's device layers point at them
    bool patched = false;        // the device layers carry table pointers (cleared again when the switch goes off)
    GeomConfig config{};
    bool seen = false;           // a launch with `seen_config` has been issued (tables are built at the second one: a batch run once never pays)
    GeomConfig seen_config{};
    bool owns = true;            // `tables` / `jobs` are this cache's to free (false: given to the device's store, or taken from it)
    bool force_build = false;    // build at the next launch whatever has been seen (a lone tick whose geometry the store has seen before)
    void *tables = nullptr;      // device: every class's tables, back to back
    void *jobs = nullptr;        // device: the precompute kernel's job list (kept: freed with the cache)
    size_t bytes = 0;
    int classes = 0;
    // the launch's layer descriptors (a batch's; a building lone tick's slot): the host copy is patched and re-sent when tables are (re)built
    DLayer *d_layers = nullptr;
    DLayer *h_layers = nullptr;
    int n_layers = 0;
};
// (Re)build the tables of the launch about to be issued on `stream` for configuration `cfg` and point its device layers at them; with the switch
// off, take the pointers out again (a cache without layer arrays only answers).  `covered`: every layer the kernels set up has its table (the
// launcher takes the CACHED kernels).
hipError_t geom_cache_prepare(GeomCache &gc, const GeomConfig &cfg, const DTick *ticks_host, int n_ticks, hipStream_t stream, bool *covered);
// frees the device memory of a cache (chv_batch_destroy; the device is current)
void geom_cache_release(GeomCache &c);

// ---- the device's STORE of tables ----------------------------------------------------------------------------------------------------
// A batch is bound to its pictures' addresses, so a host that batches builds a new batch for every group of frames and runs it once: tables owned
// by the batch would serve benchmarks only.  What recurs in a real pipeline is the GEOMETRY (a scene's layers keep their matrices and sizes for
// seconds), so a table, once built, is given to a per-device store keyed by (the class's set-up inputs, the launch configuration) and lives
// there (bounded: kGeomStoreBytes; beyond it batches keep their tables to themselves, as before).  Anything about to be launched through the
// strip kernels asks the store BEFORE its descriptors go to the device — a batch at creation, a lone tick before its descriptor slot is copied —
// and, where every staged layer has a table, gets its layers pointed at them for nothing.  A geometry seen for the second time (by any batch or
// tick of the device) is built at that launch, as a batch's second launch always did.
constexpr size_t kGeomStoreBytes = (size_t)256 << 20;
constexpr size_t kGeomStoreSightings = 8192;      // geometries asked for and not found that the store remembers (animated layers: one per tick)
// Point `layers_host` (the launch's layers, about to be copied to the device) at the store's tables: true when EVERY layer the kernels set up
// has one (the layers are patched), false otherwise (their table pointers are zeroed).  `cfg`: the launch configuration the strip kernels'
// launcher will use (n_layers = n_layers_total).  `want_build`: not covered, but every missing geometry has been seen before (or tables are
// built eagerly): worth building at this launch.  Counts the sighting.
bool geom_store_patch(int target_format, const DTick *ticks_host, DLayer *layers_host, int n_ticks, int maxW, int maxH, int n_layers_total,
                      GeomConfig *cfg, bool *want_build);
// the store of the current device in numbers (chv_debug_get_counter; tests and probes): 0 launches whose layers were all pointed at the store's
// tables before their descriptors travelled (batches at creation, lone ticks), 1 batches pointed at them at a launch, 2 builds given to the
// store, 3 bytes it holds, 4 tables (geometry classes x launch configurations) it holds
uint64_t geom_store_counter(int which);

// ---- what the strip kernels' translation unit gives the store (kernels_wave_yuv.hip.cpp) ----
// geom_precompute over `blocks` (class, strip) pairs of the job list in device memory (reports through hipGetLastError)
hipError_t launch_geom_precompute(const GeomConfig &cfg, const GeomJob *jobs, int n_jobs, int blocks, hipStream_t stream);

}  // namespace chv
