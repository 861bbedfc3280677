// What the stage drivers (pm_stage_driver.hip, rm_stage_driver.hip) share: device buffers with a guard band on either
// side, the checks of guards and read-only inputs, the dump file and its manifest, and the tiny readers of a case.
//
//   <driver> <case.json> <case.bin> <dump.json> <dump.bin>
//
// dump.bin   the buffers, appended stage by stage; dump.json says where: "entries" [{stage, name, dtype, count,
//            offset}], "derived" (a driver's own geometry), "violations" [{stage, buffer, side, offset}] -- guard bytes
//            that changed --, "inputs_changed" [names], "hip_error", "refused".
// Exit status: 0 fine, 2 case refused, 3 a HIP error or a guard violation (nothing more is launched after either),
// 4 bad usage or files.
#ifndef STAGE_DRIVER_COMMON_H
#define STAGE_DRIVER_COMMON_H
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

namespace stage_common {

constexpr size_t kGuard = 4096;      // bytes on either side of every buffer
constexpr uint8_t kCanary = 0xA5;

struct Buf {
    std::string name;
    size_t bytes = 0;
    char* base = nullptr;            // the allocation: guard | payload | guard
    bool input = false;
    std::vector<uint8_t> orig;       // an input's content
    template <class T> T* p() const { return reinterpret_cast<T*>(base + kGuard); }
};

struct Entry { std::string stage, name, dtype; size_t count, offset; };
struct Violation { std::string stage, buffer, side; size_t offset; };

inline std::vector<Buf*> g_bufs;
inline std::vector<Entry> g_entries;
inline std::vector<Violation> g_violations;
inline std::vector<std::string> g_inputs_changed;
inline std::string g_hip_error, g_refused, g_derived;
inline FILE* g_bin = nullptr;
inline size_t g_bin_at = 0;

inline bool hip_ok(hipError_t e, const char* what, const std::string& stage) {
    if (e == hipSuccess) return true;
    if (g_hip_error.empty()) g_hip_error = "stage " + stage + ": " + what + ": " + hipGetErrorString(e);
    return false;
}
#define CHK(expr) do { if (!stage_common::hip_ok((expr), #expr, stage)) return false; } while (0)

inline bool alloc(Buf& b, const char* name, size_t bytes, int fill /* payload byte */, const void* content, const std::string& stage) {
    b.name = name;
    b.bytes = bytes;
    CHK(hipMalloc((void**)&b.base, bytes + 2 * kGuard));
    CHK(hipMemset(b.base, kCanary, bytes + 2 * kGuard));
    if (content != nullptr) {
        b.input = true;
        b.orig.assign((const uint8_t*)content, (const uint8_t*)content + bytes);
        if (bytes) CHK(hipMemcpy(b.base + kGuard, content, bytes, hipMemcpyHostToDevice));
    } else if (fill != kCanary && bytes) {
        CHK(hipMemset(b.base + kGuard, fill, bytes));
    }
    g_bufs.push_back(&b);
    return true;
}

// every guard band of every buffer: the first byte that is not the canary is a violation
inline bool check_guards(const std::string& stage) {
    std::vector<uint8_t> g(kGuard);
    for (const Buf* b : g_bufs) {
        for (int side = 0; side < 2; ++side) {
            CHK(hipMemcpy(g.data(), side ? b->base + kGuard + b->bytes : b->base, kGuard, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < kGuard; ++i)
                if (g[i] != kCanary) { g_violations.push_back({stage, b->name, side ? "high" : "low", i}); break; }
        }
    }
    return true;
}

inline bool check_inputs(const std::string& stage) {
    std::vector<uint8_t> h;
    for (const Buf* b : g_bufs) {
        if (!b->input || b->bytes == 0) continue;
        h.resize(b->bytes);
        CHK(hipMemcpy(h.data(), b->base + kGuard, b->bytes, hipMemcpyDeviceToHost));
        if (std::memcmp(h.data(), b->orig.data(), b->bytes) != 0) g_inputs_changed.push_back(b->name);
    }
    return true;
}

inline bool dump(const std::string& stage, const Buf& b, const char* dtype, size_t elem, std::vector<uint8_t>* keep = nullptr) {
    std::vector<uint8_t> h(b.bytes);
    if (b.bytes) CHK(hipMemcpy(h.data(), b.base + kGuard, b.bytes, hipMemcpyDeviceToHost));
    if (b.bytes && std::fwrite(h.data(), 1, b.bytes, g_bin) != b.bytes) { g_hip_error = "stage " + stage + ": short write of the dump"; return false; }
    g_entries.push_back({stage, b.name, dtype, b.bytes / elem, g_bin_at});
    g_bin_at += b.bytes;
    if (keep) keep->swap(h);
    return true;
}

inline long long jint(const std::string& text, const char* key) {
    const size_t at = text.find(std::string("\"") + key + "\"");
    if (at == std::string::npos) { std::fprintf(stderr, "case: no key %s\n", key); std::exit(4); }
    return std::strtoll(text.c_str() + text.find(':', at) + 1, nullptr, 10);
}
inline std::string jstr(const std::string& text, const char* key) {
    const size_t at = text.find(std::string("\"") + key + "\"");
    if (at == std::string::npos) { std::fprintf(stderr, "case: no key %s\n", key); std::exit(4); }
    const size_t q0 = text.find('"', text.find(':', at) + 1);
    return text.substr(q0 + 1, text.find('"', q0 + 1) - q0 - 1);
}

inline void write_manifest(const char* path) {
    FILE* f = std::fopen(path, "w");
    if (!f) return;
    auto esc = [](const std::string& s) { std::string o; for (char ch : s) { if (ch == '"' || ch == '\\') o += '\\'; o += ch; } return o; };
    std::fprintf(f, "{\n \"derived\": {%s},\n \"entries\": [", g_derived.c_str());
    for (size_t i = 0; i < g_entries.size(); ++i)
        std::fprintf(f, "%s\n  {\"stage\": \"%s\", \"name\": \"%s\", \"dtype\": \"%s\", \"count\": %zu, \"offset\": %zu}", i ? "," : "",
                     g_entries[i].stage.c_str(), g_entries[i].name.c_str(), g_entries[i].dtype.c_str(), g_entries[i].count, g_entries[i].offset);
    std::fprintf(f, "\n ],\n \"violations\": [");
    for (size_t i = 0; i < g_violations.size(); ++i)
        std::fprintf(f, "%s\n  {\"stage\": \"%s\", \"buffer\": \"%s\", \"side\": \"%s\", \"offset\": %zu}", i ? "," : "",
                     g_violations[i].stage.c_str(), g_violations[i].buffer.c_str(), g_violations[i].side.c_str(), g_violations[i].offset);
    std::fprintf(f, "\n ],\n \"inputs_changed\": [");
    for (size_t i = 0; i < g_inputs_changed.size(); ++i) std::fprintf(f, "%s\"%s\"", i ? ", " : "", g_inputs_changed[i].c_str());
    std::fprintf(f, "],\n \"hip_error\": %s,\n \"refused\": %s\n}\n",
                 g_hip_error.empty() ? "null" : ("\"" + esc(g_hip_error) + "\"").c_str(),
                 g_refused.empty() ? "null" : ("\"" + esc(g_refused) + "\"").c_str());
    std::fclose(f);
}

template <class T> bool read_some(std::ifstream& in, std::vector<T>& v, size_t count) {
    v.resize(count);
    if (count) in.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(count * sizeof(T)));
    return (bool)in;
}

// the whole of a case's json; exits with status 4 where it cannot be read
inline std::string read_text(const char* path) {
    std::ifstream f(path);
    std::stringstream ss;
    ss << f.rdbuf();
    if (!f || ss.str().empty()) { std::fprintf(stderr, "cannot read %s\n", path); std::exit(4); }
    return ss.str();
}

// after run(): the dump's manifest, what went wrong on stderr, and the exit status
inline int finish(bool went_on, const char* manifest_path) {
    std::fclose(g_bin);
    write_manifest(manifest_path);
    if (!g_hip_error.empty()) std::fprintf(stderr, "HIP error: %s\n", g_hip_error.c_str());
    for (const Violation& v : g_violations)
        std::fprintf(stderr, "guard violation: stage %s buffer %s side %s offset %zu\n", v.stage.c_str(), v.buffer.c_str(), v.side.c_str(), v.offset);
    if (!g_refused.empty()) return 2;
    return went_on && g_hip_error.empty() && g_violations.empty() && g_inputs_changed.empty() ? 0 : 3;
}

}  // namespace stage_common
#endif
