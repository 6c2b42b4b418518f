// mz_checkpoint.cpp — checkpoints: mz_checkpoint_save / _load.
//
// Replaces `serialize(joinpath(networks_path, "$(step)_<net>.bin"), net)`
// (Learning.jl:424-431) and its `deserialize` in play.jl:12-14: Julia's
// serializer is unreadable outside Julia, so one checkpoint is one
// safetensors file (an 8-byte little-endian header length, a JSON header,
// raw little-endian data), readable from Julia (SafeTensors.jl), Python
// (safetensors, numpy) and C, and loadable without executing anything.
//
// Tensors:
//   "<net>.<i>"       the i-th array of Flux.params(<net>), <net> in
//                     representation / prediction / dynamics; its bytes are
//                     the Julia array's column-major bytes and its shape is
//                     the Julia shape reversed (the row-major view of the
//                     same bytes), e.g. a Dense W (out, in) is stored [in, out];
//   "adam.m", "adam.v"  the ADAM moments over the three nets back to back
//                     (F32, the engine's flat order = the nets' Flux order);
//   "adam.beta_pow"   (β1^t, β2^t) (F64), the optimiser's βp state.
// __metadata__: format, network ("fc" | "resnet"), training_step, config
// (JSON).  Loading checks every parameter's shape against this engine.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "mz_ckpt_iface.h"
#include "mz_st_header.h"

namespace {

std::string esc(const std::string& s) {
    std::string o;
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o;
}

struct Entry {
    std::string name, dtype;
    std::vector<int64_t> shape;   // safetensors (row-major) shape
    const void* data;
    size_t bytes;
};

// an open safetensors file: the parsed header, and reads of named tensors checked against the
// dtype and shape the caller expects; every call returns "" or the error
struct StFile {
    std::unique_ptr<FILE, int (*)(FILE*)> f{nullptr, std::fclose};
    uint64_t hl = 0;
    long long fsize = 0;
    mzst::JV root;

    std::string open(const char* path) {
        f.reset(std::fopen(path, "rb"));
        if (!f) return std::string("cannot open ") + path;
        if (std::fread(&hl, 8, 1, f.get()) != 1 || hl > (1u << 28)) return "not a safetensors file";
        std::string hdr(hl, '\0');
        if (std::fread(&hdr[0], 1, hl, f.get()) != hl) return "truncated header";
        const std::string perr = mzst::parse_header(hdr.data(), hdr.size(), &root);
        if (!perr.empty()) return perr;
        std::fseek(f.get(), 0, SEEK_END);
        fsize = std::ftell(f.get());
        return "";
    }
    std::string read(const std::string& name, const char* dtype, size_t esz, std::vector<int64_t> shape, void* dst) {
        long long off = 0;
        const std::string err = mzst::entry_span(root, name, dtype, esz, shape, hl, fsize, &off);
        if (!err.empty()) return err;
        size_t cnt = 1;
        for (int64_t d : shape) cnt *= (size_t)d;
        std::fseek(f.get(), (long)off, SEEK_SET);
        if (std::fread(dst, 1, cnt * esz, f.get()) != cnt * esz) return name + ": short read";
        return "";
    }
    // the three nets' Flux.params arrays into flat (the engine's flat order), every shape checked
    std::string read_nets(const mz_handle* h, float* flat) {
        for (const MzParamDesc& d : mz_param_table(h)) {
            std::vector<int64_t> shp(d.jshape.rbegin(), d.jshape.rend());
            const std::string e = read(d.name, "F32", 4, shp, flat + d.off);
            if (!e.empty()) return e;
        }
        return "";
    }
    std::string meta(const char* key) const {          // a __metadata__ string, "" if absent
        auto md = root.obj.find("__metadata__");
        if (md == root.obj.end() || md->second.t != mzst::JV::OBJ) return "";
        auto it = md->second.obj.find(key);
        return it != md->second.obj.end() && it->second.t == mzst::JV::STR ? it->second.str : "";
    }
    int64_t training_step() const { return std::strtoll(meta("training_step").c_str(), nullptr, 10); }
};

}  // namespace

extern "C" {

int mz_checkpoint_save(mz_handle* h, const char* path, int64_t training_step) {
    if (!h) return -2;
    if (!path) return mz_set_error(h, "null path");
    const size_t n = mz_flat_count(h);
    std::vector<float> flat(n), m(n), v(n);
    double bp[2];
    if (mz_state_get(h, flat.data(), m.data(), v.data(), bp)) return -1;
    std::vector<Entry> ents;
    for (const MzParamDesc& d : mz_param_table(h)) {
        std::vector<int64_t> shp(d.jshape.rbegin(), d.jshape.rend());
        ents.push_back(Entry{d.name, "F32", shp, flat.data() + d.off, d.count * 4});
    }
    ents.push_back(Entry{"adam.m", "F32", {(int64_t)n}, m.data(), n * 4});
    ents.push_back(Entry{"adam.v", "F32", {(int64_t)n}, v.data(), n * 4});
    ents.push_back(Entry{"adam.beta_pow", "F64", {2}, bp, 16});
    std::string hdr = "{\"__metadata__\":{\"format\":\"libmz-checkpoint-1\",\"network\":\"" + mz_net_kind(h) +
                      "\",\"training_step\":\"" + std::to_string((long long)training_step) + "\",\"config\":\"" +
                      esc(mz_describe(h)) + "\"}";
    size_t off = 0;
    for (const Entry& e : ents) {
        hdr += ",\"" + e.name + "\":{\"dtype\":\"" + e.dtype + "\",\"shape\":[";
        for (size_t i = 0; i < e.shape.size(); ++i) hdr += (i ? "," : "") + std::to_string((long long)e.shape[i]);
        hdr += "],\"data_offsets\":[" + std::to_string(off) + "," + std::to_string(off + e.bytes) + "]}";
        off += e.bytes;
    }
    hdr += "}";
    while (hdr.size() % 8) hdr += ' ';
    const std::string tmp = std::string(path) + ".tmp";
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) return mz_set_error(h, std::string("cannot write ") + tmp);
    const uint64_t hl = hdr.size();
    bool ok = std::fwrite(&hl, 8, 1, f) == 1 && std::fwrite(hdr.data(), 1, hdr.size(), f) == hdr.size();
    for (const Entry& e : ents) ok = ok && std::fwrite(e.data, 1, e.bytes, f) == e.bytes;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path) != 0) {
        std::remove(tmp.c_str());
        return mz_set_error(h, std::string("writing ") + path + " failed");
    }
    return 0;
}

int mz_checkpoint_load(mz_handle* h, const char* path, int64_t* training_step) {
    if (!h) return -2;
    if (!path) return mz_set_error(h, "null path");
    StFile sf;
    if (const std::string e = sf.open(path); !e.empty()) return mz_set_error(h, e);
    const size_t n = mz_flat_count(h);
    std::vector<float> flat(n), m(n), v(n);
    double bp[2];
    std::string e = sf.read_nets(h, flat.data());
    if (e.empty()) e = sf.read("adam.m", "F32", 4, {(int64_t)n}, m.data());
    if (e.empty()) e = sf.read("adam.v", "F32", 4, {(int64_t)n}, v.data());
    if (e.empty()) e = sf.read("adam.beta_pow", "F64", 8, {2}, bp);
    if (!e.empty()) return mz_set_error(h, e);
    if (training_step) *training_step = sf.training_step();
    return mz_state_set(h, flat.data(), m.data(), v.data(), bp);
}

// The opponent's weight set of MZ_OPP_NETWORK from a checkpoint or a snapshot (a superset of one):
// only the three nets' arrays are read, by name; the file is validated whole before the set changes.
int mz_opponent_load(mz_handle* h, const char* path, int64_t* training_step) {
    if (!h) return -2;
    if (!path) return mz_set_error(h, "null path");
    StFile sf;
    if (const std::string e = sf.open(path); !e.empty()) return mz_set_error(h, e);
    const std::string kind = sf.meta("network");
    if (kind != mz_net_kind(h))
        return mz_set_error(h, "opponent_load: the file's network is \"" + kind + "\", this engine's is \"" +
                                   mz_net_kind(h) + "\"");
    std::vector<float> flat(mz_flat_count(h));
    if (const std::string e = sf.read_nets(h, flat.data()); !e.empty()) return mz_set_error(h, "opponent_load: " + e);
    if (training_step) *training_step = sf.training_step();
    return mz_opponent_put(h, flat.data());
}

}  // extern "C"
