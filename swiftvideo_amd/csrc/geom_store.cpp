// geom_store.cpp — the host side of the strip kernels' geometry tables (geom_cache.h): a launch's tables built, given to the device's store and
// found there, the layers pointed at them.  The launch configuration comes from the route unit (tick_route.cpp: wave_geom_config); of the kernels'
// translation unit it takes one thing (kernels_wave_yuv.hip.cpp): the launch of the kernel that fills the tables (launch_geom_precompute).
#include "geom_cache.h"
#include "tick_route.h"
#include "switches.h"

#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

namespace chv {

void geom_cache_release(GeomCache &c) {
    if (c.owns) {
        if (c.tables) (void)hipFree(c.tables);
        if (c.jobs) (void)hipFree(c.jobs);
    }
    c.tables = c.jobs = nullptr;
    c.owns = true;
    c.built = false; c.bytes = 0; c.classes = 0;
}

// ---- the device's store (geom_cache.h) ----
struct GeomStore {
    std::mutex mu;
    std::unordered_map<std::string, void *> tables;          // (class key + configuration key) -> the class's table
    std::unordered_map<std::string, int> sightings;          // launches that asked for it and did not find it
    std::vector<void *> owned;                               // allocations given to the store (never freed: the store lives as long as the process)
    size_t bytes = 0;
    bool full = false;                                       // a build did not fit any more: nothing asks for builds on the store's behalf from here on
    std::atomic<uint64_t> patched{0};                        // (geom_store_counter; bumped without the lock by the lone tick's memo)
    uint64_t batch_hits = 0, builds = 0;
};
static GeomStore &geom_store() {
    static GeomStore *const stores = new GeomStore[16];      // (never destroyed either: what it owns stays reachable until the process ends)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
    return stores[dev & 15];
}
uint64_t geom_store_counter(int which) {
    GeomStore &st = geom_store();
    std::lock_guard<std::mutex> lk(st.mu);
    switch (which) {
    case 0: return st.patched.load(std::memory_order_relaxed);
    case 1: return st.batch_hits;
    case 2: return st.builds;
    case 3: return (uint64_t)st.bytes;
    case 4: return (uint64_t)st.tables.size();
    }
    return 0;
}
// the inputs of a layer's set-up as bytes: the three matrices, the source planes' sizes and layout class, the canvas size (false: the layer is
// applied per pixel — no set-up, no table)
struct GeomRawKey { float u[48]; int32_t w0, h0, w1, h1, cls, W, H; };
static bool geom_class_raw(const DTick &T, const DLayer &L, GeomRawKey &k) {
    if (L.kind == LK_BGRA_METAL || (L.flags & (LF_AXIS_ALIGNED | LF_BOUNDED)) != (LF_AXIS_ALIGNED | LF_BOUNDED)) return false;
    memset(&k, 0, sizeof k);
    memcpy(k.u, L.u, sizeof k.u);
    const bool rgb = L.kind == LK_BGRA_FROM_RGB || L.kind == LK_YUV_FROM_RGB || L.kind == LK_YUV_FROM_RGB_INT;
    k.w0 = L.src.pl[0].w; k.h0 = L.src.pl[0].h; k.w1 = rgb ? 0 : L.src.pl[1].w; k.h1 = rgb ? 0 : L.src.pl[1].h;
    k.cls = rgb ? 2 : (L.kind == LK_BGRA_FROM_Y420P || L.kind == LK_YUV_FROM_Y420P) ? 1 : 0; k.W = T.W; k.H = T.H;
    return true;
}
// The scene a thread's last covered LONE tick was (its classes' raw keys, the launch configuration, the tables): the next tick of the scene —
// the steady state of a mixer — compares bytes and takes the pointers; no strings, no hashing, no lock (tables are never freed, so a covered
// answer stays right).  0.6 us of a lone tick's 4.8 us of host time (tools/host_enqueue_probe.py).
struct GeomLoneMemo { int dev = -1, n = 0, tf = -1; GeomConfig cfg{}; bool has[WAVE_ONE_LAYERS + 2]; GeomRawKey key[WAVE_ONE_LAYERS + 2]; void *tab[WAVE_ONE_LAYERS + 2]; };
static GeomLoneMemo &geom_lone_memo() {
    static thread_local GeomLoneMemo m;
    return m;
}
// what of a launch configuration a class's table depends on (everything but the size of the batch's layer array)
static std::string geom_config_key(const GeomConfig &c) {
    const int32_t v[9] = { c.target_format, c.wth, c.p0pitch, c.p0rows, c.p1pitch, c.p1rows, c.planar_any, c.strips_x, c.strips_y };
    return std::string((const char *)v, sizeof v);
}

static hipError_t geom_send_layers(const GeomCache &gc) {
    return hipMemcpy(gc.d_layers, gc.h_layers, sizeof(DLayer) * (size_t)gc.n_layers, hipMemcpyHostToDevice);
}
// Take the table pointers out of the batch's device layers.  Nothing in flight may still read the layers: wait, then copy synchronously.
static hipError_t geom_cache_unpatch(GeomCache &gc, hipStream_t stream) {
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    for (int i = 0; i < gc.n_layers; i++) geom_set_table(gc.h_layers[i], nullptr);
    e = geom_send_layers(gc);
    if (e == hipSuccess) gc.patched = gc.built = false;
    return e;
}

// Everything is ordered on `stream` in front of the tick kernel.
hipError_t geom_cache_prepare(GeomCache &gc, const GeomConfig &cfg, const DTick *ticks_host, int n_ticks, hipStream_t stream, bool *covered) {
    DLayer *hl = gc.h_layers;
    // no layer arrays: a lone tick whose layers the store pointed at its tables (geom_store_patch) before they travelled, for exactly `config`
    if (!hl || !gc.d_layers || gc.n_layers <= 0) { *covered = gc.built && gc.patched && gc.config == cfg; return hipSuccess; }
    *covered = false;
    const bool on = CHV_GEOM_CACHE && switches().geom_cache.load(std::memory_order_relaxed) != 0;
    if (!on) return gc.patched ? geom_cache_unpatch(gc, stream) : hipSuccess;      // (rare: a switch flipped between two runs of a batch)
    if (gc.built && gc.config == cfg) { *covered = gc.patched; return hipSuccess; }
    // classes: layers whose set-up inputs are the same bytes — the three matrices, the source planes' sizes and layout class, the canvas size
    std::map<std::string, int> index;
    std::vector<GeomJob> jobs;
    std::vector<std::string> keys;
    std::vector<int> cls_of((size_t)gc.n_layers, -1);
    for (int i = 0; i < n_ticks; i++) {
        const DTick &T = ticks_host[i];
        for (int l = 0; l < T.n_layers; l++) {
            const int li = T.first_layer + l;
            if (li < 0 || li >= gc.n_layers) continue;
            const DLayer &L = hl[li];
            GeomRawKey rk;
            if (!geom_class_raw(T, L, rk)) continue;             // applied per pixel: no set-up
            const std::string ks((const char *)&rk, sizeof rk);
            auto it = index.find(ks);
            if (it == index.end()) {
                GeomJob J;
                memset(&J, 0, sizeof J);
                J.layer = L;
                geom_set_table(J.layer, nullptr);
                J.W = T.W; J.H = T.H;
                J.strips_x = (T.W + WTW - 1) / WTW; J.strips_y = (T.H + cfg.wth - 1) / cfg.wth;
                it = index.emplace(ks, (int)jobs.size()).first;
                jobs.push_back(J);
                keys.push_back(ks);
            }
            cls_of[(size_t)li] = it->second;
        }
    }
    // The device's store first: tables another batch (or lone tick) of this geometry and configuration left there.  All found: the layers are
    // pointed at them (one drain + one copy of the layer array, no allocation, no kernel) whatever this batch has seen.
    const std::string ck = geom_config_key(cfg);
    bool known = !jobs.empty();                 // every class has been asked for before (by anything on this device)
    GeomStore &st = geom_store();
    {
        std::vector<void *> found(jobs.size(), nullptr);
        bool all = !jobs.empty() && jobs.size() <= 256;
        {
            std::lock_guard<std::mutex> lk(st.mu);
            for (size_t c = 0; c < jobs.size(); c++) {
                const std::string full = keys[c] + ck;
                auto it = st.tables.find(full);
                if (it != st.tables.end()) found[c] = it->second; else all = false;
                auto sg = st.sightings.find(full);
                if (sg == st.sightings.end() || sg->second < 2 || st.full) known = false;
            }
        }
        if (all) {
            hipError_t es = hipStreamSynchronize(stream);
            if (es != hipSuccess) return es;
            geom_cache_release(gc);
            for (int i = 0; i < gc.n_layers; i++) geom_set_table(hl[i], cls_of[(size_t)i] < 0 ? nullptr : found[(size_t)cls_of[(size_t)i]]);
            es = geom_send_layers(gc);
            if (es != hipSuccess) return es;
            gc.owns = false; gc.tables = found[0]; gc.patched = true; gc.built = true; gc.config = cfg; gc.classes = (int)jobs.size();
            { std::lock_guard<std::mutex> lk(st.mu); st.batch_hits++; }
            *covered = true;
            return hipSuccess;
        }
    }
    // A batch that is run once (a host that builds one per tick) never pays for tables: they are built at the SECOND launch with a configuration
    // (draining the stream, three small copies and a kernel: tens of microseconds) — the second launch of this batch, or a launch of geometry the
    // store has been asked for before —, the first one computes its geometry in place.
    if (!(gc.seen && gc.seen_config == cfg) && !gc.force_build && !known && switches().geom_cache.load(std::memory_order_relaxed) != 2) {
        gc.seen = true; gc.seen_config = cfg;
        // (tables of another configuration: the kernels about to run compute in place and never look, but the pointers go)
        return gc.patched ? geom_cache_unpatch(gc, stream) : hipSuccess;
    }
    // A (re)build happens once per batch and launch configuration: an earlier run of the batch may still be reading the layers, and the host
    // buffers below are pageable — the stream is drained first and every copy is a synchronous one (an asynchronous copy from pageable memory
    // may read its source after this function has returned).
    hipError_t e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    geom_cache_release(gc);
    for (int i = 0; i < gc.n_layers; i++) geom_set_table(hl[i], nullptr);
    // (a batch of a thousand distinct geometries gains nothing from tables that are each used once)
    if (!jobs.empty() && jobs.size() <= 256) {
        const size_t row_bytes = (size_t)2 * 3 * cfg.wth * 16 + 64;      // the staged and the unstaged row table, 16 scalars
        std::vector<GeomHdr> hdr(jobs.size());
        std::vector<size_t> offs(jobs.size());
        size_t total = 0;
        int blocks = 0;
        for (size_t c = 0; c < jobs.size(); c++) {
            GeomJob &J = jobs[c];
            GeomHdr &H = hdr[c];
            memset(&H, 0, sizeof H);
            H.strips_x = J.strips_x; H.strips_y = J.strips_y; H.wth = cfg.wth; H.row_bytes = (int32_t)row_bytes;
            H.flags_off = (uint32_t)sizeof(GeomHdr);
            H.cols_off = H.flags_off + (uint32_t)(((size_t)J.strips_x * J.strips_y * 4 + 15) & ~(size_t)15);
            H.rows_off = H.cols_off + (uint32_t)((size_t)J.strips_x * kGeomColBytes);
            offs[c] = total;
            total = (total + H.rows_off + (size_t)J.strips_y * row_bytes + 255) & ~(size_t)255;
            J.first_block = blocks;
            blocks += J.strips_x * J.strips_y;
        }
        e = hipMalloc(&gc.tables, total);
        if (e == hipSuccess) e = hipMalloc(&gc.jobs, sizeof(GeomJob) * jobs.size());

        if (e == hipSuccess) {
            std::vector<uint8_t> image(total, 0);              // zeroed: a strip's flag word 0 = "not in the table"
            for (size_t c = 0; c < jobs.size(); c++) {
                jobs[c].table = (uint8_t *)gc.tables + offs[c];
                memcpy(image.data() + offs[c], &hdr[c], sizeof(GeomHdr));
            }
            e = hipMemcpy(gc.tables, image.data(), total, hipMemcpyHostToDevice);
        }
        if (e == hipSuccess) e = hipMemcpy(gc.jobs, jobs.data(), sizeof(GeomJob) * jobs.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            (void)hipGetLastError();
            e = launch_geom_precompute(cfg, (const GeomJob *)gc.jobs, (int)jobs.size(), blocks, stream);
        }
        if (e == hipSuccess) {
            for (int i = 0; i < gc.n_layers; i++)
                if (cls_of[(size_t)i] >= 0) geom_set_table(hl[i], jobs[(size_t)cls_of[(size_t)i]].table);
            gc.bytes = total; gc.classes = (int)jobs.size();
            gc.owns = true;
            // The tables go to the device's store (another stream may read them: the precompute kernel has to be done first).
            if (hipStreamSynchronize(stream) == hipSuccess) {
                std::lock_guard<std::mutex> lk(st.mu);
                const size_t give = total + sizeof(GeomJob) * jobs.size();
                if (st.bytes + give <= kGeomStoreBytes) {
                    for (size_t c = 0; c < jobs.size(); c++) st.tables.emplace(keys[c] + ck, (void *)jobs[c].table);      // (a class another thread gave meanwhile keeps its first table)
                    st.owned.push_back(gc.tables); st.owned.push_back(gc.jobs);
                    st.bytes += give;
                    st.builds++;
                    gc.owns = false;
                } else st.full = true;
            } else (void)hipGetLastError();
        } else {
            (void)hipGetLastError();
            geom_cache_release(gc);             // no tables: the kernels compute their geometry as before
            e = hipSuccess;
        }
    }
    hipError_t e2 = geom_send_layers(gc);
    if (e2 != hipSuccess) return e2;
    gc.patched = gc.tables != nullptr;        // (every layer the kernels set up has a table, or none has: classes are all-or-nothing)
    gc.built = true;
    gc.force_build = false;
    gc.config = cfg;
    *covered = gc.patched;
    return e;
}

bool geom_store_patch(int target_format, const DTick *ticks_host, DLayer *layers_host, int n_ticks, int maxW, int maxH, int n_layers_total,
                      GeomConfig *cfg_out, bool *want_build) {
    *want_build = false;
    const int mode = CHV_GEOM_CACHE ? switches().geom_cache.load(std::memory_order_relaxed) : 0;
    if (n_ticks < 1 || !layers_host) return false;
    const bool takes_tables = wave_geom_config(target_format, ticks_host, layers_host, n_ticks, maxW, maxH, n_layers_total, cfg_out);
    auto zero = [&]() {
        for (int i = 0; i < n_ticks; i++)
            for (int l = 0; l < ticks_host[i].n_layers; l++) geom_set_table(layers_host[ticks_host[i].first_layer + l], nullptr);
    };
    if (!mode || !takes_tables) { zero(); return false; }        // (off; launches of RGB layers only keep computing in place; nothing staged)
    // a lone tick of the scene this thread's last covered lone tick was
    constexpr int MEMO_MAX = WAVE_ONE_LAYERS + 2;
    const bool lone = n_ticks == 1 && ticks_host[0].n_layers >= 1 && ticks_host[0].n_layers <= MEMO_MAX;
    GeomRawKey raw[MEMO_MAX];
    bool has[MEMO_MAX];
    int dev = 0;
    if (lone) {
        if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); dev = 0; }
        const DTick &T = ticks_host[0];
        for (int l = 0; l < T.n_layers; l++) has[l] = geom_class_raw(T, layers_host[T.first_layer + l], raw[l]);
        GeomLoneMemo &m = geom_lone_memo();
        bool same = m.dev == dev && m.n == T.n_layers && m.tf == target_format && m.cfg == *cfg_out;
        for (int l = 0; same && l < T.n_layers; l++) same = m.has[l] == has[l] && (!has[l] || memcmp(&m.key[l], &raw[l], sizeof raw[l]) == 0);
        if (same) {
            for (int l = 0; l < T.n_layers; l++) geom_set_table(layers_host[T.first_layer + l], has[l] ? m.tab[l] : nullptr);
            geom_store().patched.fetch_add(1, std::memory_order_relaxed);
            return true;
        }
    }
    const std::string ck = geom_config_key(*cfg_out);
    GeomStore &st = geom_store();
    std::vector<std::pair<int, void *>> hits;
    bool all = true, known = true;
    {
        std::lock_guard<std::mutex> lk(st.mu);
        // this call's classes (a sighting is a LAUNCH that asked, whatever its number of ticks): the first sixteen as raw keys compared by bytes,
        // starting from where the same layer of the previous tick was found (a group's ticks repeat their predecessor's geometry: one memcmp
        // per layer — a batch of 128 mixer ticks used to pay 27 us of strings and hashing here); further ones through a map
        struct Seen { GeomRawKey k; void *tab; };
        Seen seen[16];
        int n_seen = 0;
        std::string ks;
        std::unordered_map<std::string, void *> asked;
        auto lookup = [&](const std::string &key) -> void * {
            const std::string full = key + ck;
            auto it = st.tables.find(full);
            void *tab = it != st.tables.end() ? it->second : nullptr;
            if (!tab) {
                // (an animated layer is a new geometry every tick, seen once: the count of sightings is bounded by starting over)
                if (st.sightings.size() >= kGeomStoreSightings) st.sightings.clear();
                int &n = st.sightings[full];
                if (n < (1 << 20)) n++;
                if (n < 2 || st.full) known = false;
            }
            return tab;
        };
        for (int i = 0; i < n_ticks; i++) {
            const DTick &T = ticks_host[i];
            for (int l = 0; l < T.n_layers; l++) {
                const int li = T.first_layer + l;
                GeomRawKey rk;
                if (!geom_class_raw(T, layers_host[li], rk)) continue;
                void *tab = nullptr;
                int at = -1;
                for (int q = 0; q < n_seen && at < 0; q++) {
                    const int j = (l + q) % n_seen;                  // (layer l of a tick is usually class l of the group)
                    if (memcmp(&seen[j].k, &rk, sizeof rk) == 0) at = j;
                }
                if (at >= 0) tab = seen[at].tab;
                else {
                    ks.assign((const char *)&rk, sizeof rk);
                    if (n_seen < 16) {
                        tab = lookup(ks);
                        seen[n_seen].k = rk; seen[n_seen].tab = tab; n_seen++;
                    } else {
                        auto f = asked.find(ks);
                        if (f != asked.end()) tab = f->second;
                        else { tab = lookup(ks); asked.emplace(ks, tab); }
                    }
                }
                if (tab) hits.emplace_back(li, tab); else all = false;
            }
        }
    }
    zero();
    if (!all || hits.empty()) {
        *want_build = !all && (known || mode == 2);          // (!all: a class was looked up and not found)
        return false;
    }
    st.patched.fetch_add(1, std::memory_order_relaxed);
    for (auto &h : hits) geom_set_table(layers_host[h.first], h.second);
    if (lone) {
        GeomLoneMemo &m = geom_lone_memo();
        const DTick &T = ticks_host[0];
        m.dev = dev; m.n = T.n_layers; m.tf = target_format; m.cfg = *cfg_out;
        for (int l = 0; l < T.n_layers; l++) {
            m.has[l] = has[l];
            if (has[l]) m.key[l] = raw[l];
            m.tab[l] = geom_table(layers_host[T.first_layer + l]);
        }
    }
    return true;
}

}  // namespace chv
