// Launch recorder (diagnostics, like vc_detect_debug_layer): armed for the next detector or ReID pass, it keeps for every launch
// run_ops_body makes what a test needs to recompute that launch alone -- the ops it covered with every ConvP / View field, the bytes of
// every buffer it reads (copied just before the launch) and of every buffer it writes (copied before and after), all on the stream the
// launch runs on.  tests/graph_launch_cases.py turns a record into a float64 reference of the launch on its own input.
//
// Unarmed, run_ops_body tests one pointer per launch and nothing is allocated.  The arena is sized from the plan when an armed pass
// begins and is freed with the engine.
#include <cstdarg>

#include "engine.h"

namespace vc {

struct RecBuf {
    const void* ptr; std::string name;
    int es, cs; size_t bytes; bool written;
    size_t before = 0, after = 0;            // arena offsets
};
struct RecLaunch { int net, op0, n_ops, cfg, side; std::string ops; std::vector<RecBuf> bufs; };
struct LaunchRecorder {
    char* d_arena = nullptr; size_t cap = 0, used = 0;
    std::vector<RecLaunch> launches;
    std::map<const void*, std::string> names;
    const Net* net = nullptr; int net_id = 0;
    const Op* ops0 = nullptr;                // first op of the plan being recorded
};

static void jf(std::string& s, const char* fmt, ...) {
    char b[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(b, sizeof(b), fmt, ap);
    va_end(ap);
    s += b;
}

static size_t view_bytes(size_t rows, int cs, int es) { return rows * (size_t)cs * es; }

// the arena an armed pass can need: every view of every op twice (a written buffer is copied before and after), the u8 frames, the counters
static size_t plan_bytes(vc_engine* e, const std::vector<Op>& ops) {
    size_t t = (size_t)e->cfg.max_batch * e->cfg.max_frame_h * e->cfg.max_frame_w * 3 + 4096;
    auto add = [&](size_t rows, int cs, int es) { t += 2 * (view_bytes(rows, cs, es) + 256); };
    for (const Op& op : ops) {
        if (op.kind == Op::CONV) {
            const ConvP& c = op.conv;
            const size_t in_rows = (size_t)c.B * c.H * c.W;
            add(in_rows, c.in_cs, 4); add(in_rows, c.in_cs, 4);          // (the second: a folded upsample's source is never larger)
            if (c.res) add(c.M, c.res_cs, 4);
            add(c.M, c.out_cs, 4);
            if (c.split) add(c.M, c.out2_cs, 4);
        } else if (op.kind == Op::HEAD_COMPACT) {
            const size_t M = (size_t)op.a.B * op.a.H * op.a.W;
            add(M, 8, 2); add(M, op.a.cs, 2); add(e->hc_cap[op.level], op.a.C, 2); add(e->hc_cap[op.level], 1, 4); add(64, 1, 4);
        } else {
            add((size_t)op.a.B * op.a.H * op.a.W, op.a.cs, 4);
            if (op.b.ptr) add((size_t)op.b.B * op.b.H * op.b.W, op.b.cs, 4);
        }
    }
    return t;
}

int record_begin(vc_engine* e, int net, const std::vector<Op>& ops, LaunchRecorder** out) {
    *out = nullptr;
    if (e->rec_armed != net + 1) return VC_OK;
    e->rec_armed = 0;
    if (!e->rec) e->rec = new LaunchRecorder();
    LaunchRecorder* r = e->rec;
    const size_t need = plan_bytes(e, ops);
    if (need > r->cap) {
        VC_HIP(hipDeviceSynchronize());
        if (r->d_arena) (void)hipFree(r->d_arena);
        r->d_arena = nullptr; r->cap = 0;
        VC_HIP(hipMalloc((void**)&r->d_arena, need));
        r->cap = need;
    }
    r->used = 0; r->launches.clear(); r->names.clear();
    r->net = net == VC_NET_YOLO ? &e->yolo : &e->reid; r->net_id = net; r->ops0 = ops.data();
    for (const auto& kv : (net == VC_NET_YOLO ? e->ybuf : e->rbuf)) r->names[kv.second.ptr] = kv.first;
    if (net == VC_NET_YOLO) {
        for (int i = 0; i < 3; ++i) {
            const std::string n = std::to_string(i);
            r->names[e->d_logits[i]] = "logits" + n;
            if (e->d_obj[i]) { r->names[e->d_obj[i]] = "obj" + n; r->names[e->d_hc_list[i]] = "hc_list" + n; r->names[e->d_hc_x[i]] = "hc_x" + n; r->names[e->d_hc_logits[i]] = "hc_logits" + n; }
        }
        // one buffer per level's counter: a launch copies its own 4 bytes only (the P3 / P4 head ops run on the head stream beside the main
        // stream's P5 compaction, which must not show up between their two copies)
        if (e->d_hc_count) for (int i = 0; i < 3; ++i) r->names[e->d_hc_count + i] = "hc_count" + std::to_string(i);
        r->names[e->post.overflow] = "overflow";
    }
    *out = r;
    return VC_OK;
}

void record_free(vc_engine* e) {
    if (!e->rec) return;
    if (e->rec->d_arena) (void)hipFree(e->rec->d_arena);
    delete e->rec;
    e->rec = nullptr;
}

namespace {
struct Describe {
    vc_engine* e; LaunchRecorder* r; RecLaunch& L;
    int buf(const void* ptr, size_t bytes, int cs, int es, bool written, const char* fallback = nullptr) {
        for (size_t i = 0; i < L.bufs.size(); ++i)
            if (L.bufs[i].ptr == ptr) { L.bufs[i].bytes = std::max(L.bufs[i].bytes, bytes); L.bufs[i].written |= written; return (int)i; }
        RecBuf b{};
        b.ptr = ptr; b.es = es; b.cs = cs; b.bytes = bytes; b.written = written;
        auto it = r->names.find(ptr);
        b.name = it != r->names.end() ? it->second : (fallback ? fallback : "?");
        L.bufs.push_back(b);
        return (int)L.bufs.size() - 1;
    }
    void view(std::string& s, const char* key, const void* ptr, size_t rows, int cs, int co, int C, int es, bool written) {
        jf(s, "\"%s\":{\"buf\":%d,\"rows\":%zu,\"cs\":%d,\"co\":%d,\"C\":%d,\"es\":%d},", key, buf(ptr, view_bytes(rows, cs, es), cs, es, written), rows, cs, co, C, es);
    }
    void view(std::string& s, const char* key, const View& v, int es, bool written) {
        jf(s, "\"%s\":{\"buf\":%d,\"B\":%d,\"H\":%d,\"W\":%d,\"cs\":%d,\"co\":%d,\"C\":%d,\"es\":%d},", key,
           buf(v.ptr, view_bytes((size_t)v.B * v.H * v.W, v.cs, es), v.cs, es, written), v.B, v.H, v.W, v.cs, v.co, v.C, es);
    }
    void conv(std::string& s, const Op& op, const ConvP& c, bool u8_src) {
        const ConvParam& p = r->net->params[op.param];
        const int es = elem_size(c.prec), oes = c.out_f32 ? 4 : (c.out_bf16 ? 2 : es);
        jf(s, "{\"kind\":\"conv\",\"param\":\"%s\",\"pair_stem\":%d,\"B\":%d,\"H\":%d,\"W\":%d,\"Cin\":%d,\"Cout\":%d,\"cout_logical\":%d,", p.name.c_str(), p.pair_stem ? 1 : 0,
           c.B, c.H, c.W, c.Cin, c.Cout, op.cout_logical);
        jf(s, "\"kh\":%d,\"kw\":%d,\"sh\":%d,\"sw\":%d,\"ph\":%d,\"pw\":%d,\"Ho\":%d,\"Wo\":%d,\"act\":%d,\"res_mode\":%d,\"prec\":%d,\"out_f32\":%d,\"out_bf16\":%d,\"split\":%d,\"M\":%d,"
              "\"act_scale\":%.9g,", c.kh, c.kw, c.sh, c.sw, c.ph, c.pw, c.Ho, c.Wo, c.act, c.res_mode, c.prec, c.out_f32, c.out_bf16, c.split, c.M, (double)c.act_scale);
        const size_t in_rows = (size_t)c.B * c.H * c.W;
        view(s, "in", c.in, in_rows, c.in_cs, c.in_co, c.Cin, es, false);
        if (c.res) view(s, "res", c.res, c.M, c.res_cs, c.res_co, c.Cout, es, false);
        if (c.in_up) view(s, "up", c.in_up, in_rows / 4, c.up_cs, c.up_co, c.up_C, es, false);
        view(s, "out", c.out, c.M, c.out_cs, c.out_co, c.split ? c.split : c.Cout, oes, true);
        if (c.split) view(s, "out2", c.out2, c.M, c.out2_cs, c.out2_co, c.Cout - c.split, oes, true);
        if (c.m_dev) jf(s, "\"m_dev\":{\"buf\":%d,\"index\":%d},", buf(c.m_dev, 4, 1, 4, false), 0);
        if (u8_src) {
            const LetterboxGeom& g = e->stem_geom;
            jf(s, "\"u8\":{\"buf\":%d,\"src_h\":%d,\"src_w\":%d,\"net_h\":%d,\"net_w\":%d,\"unpad_h\":%d,\"unpad_w\":%d,\"top\":%d,\"left\":%d,\"swap_rb\":%d},",
               buf(e->stem_src, (size_t)c.B * g.src_h * g.src_w * 3, 3, 1, false, "frames"), g.src_h, g.src_w, g.net_h, g.net_w, g.unpad_h, g.unpad_w, g.top, g.left, g.swap_rb);
        }
        jf(s, "\"K\":%d}", c.K);
    }
    void op(std::string& s, const Op& o, const ConvP* cp, bool u8_src) {
        switch (o.kind) {
            case Op::CONV: conv(s, o, cp ? *cp : o.conv, u8_src); break;
            case Op::SPPF:
                s += "{\"kind\":\"sppf\","; view(s, "a", o.a, elem_size(e->prec), true); jf(s, "\"C\":%d}", o.C); break;
            case Op::UPSAMPLE:
                s += "{\"kind\":\"upsample\","; view(s, "a", o.a, elem_size(e->prec), false); view(s, "b", o.b, elem_size(e->prec), true); s += "\"x\":0}"; break;
            case Op::MAXPOOL:
                s += "{\"kind\":\"maxpool\","; view(s, "a", o.a, elem_size(e->aux_prec), false); view(s, "b", o.b, elem_size(e->aux_prec), true); s += "\"x\":0}"; break;
            case Op::TO_FP8:
                s += "{\"kind\":\"to_fp8\","; view(s, "a", o.a, 2, false); view(s, "b", o.b, 1, true); jf(s, "\"inv_scale\":%.9g}", (double)(1.0f / e->act_scale)); break;
            case Op::HEAD_COMPACT: {
                const int i = o.level, M = o.a.B * o.a.H * o.a.W, cap = e->hc_cap[i];
                jf(s, "{\"kind\":\"head_compact\",\"level\":%d,\"M\":%d,\"pix_per_frame\":%d,\"conf\":%.9g,\"cap\":%d,", i, M, o.a.H * o.a.W, (double)e->cfg.conf_thres, cap);
                view(s, "obj", e->d_obj[i], (size_t)M, 8, 0, 8, 2, false);
                view(s, "a", o.a, 2, false);
                jf(s, "\"count\":{\"buf\":%d,\"index\":%d},", buf(e->d_hc_count + i, 4, 1, 4, true), 0);
                view(s, "list", e->d_hc_list[i], (size_t)cap, 1, 0, 1, 4, true);
                view(s, "xc", e->d_hc_x[i], (size_t)cap, o.a.C, 0, o.a.C, 2, true);
                view(s, "overflow", e->post.overflow, (size_t)o.a.B, 1, 0, 1, 4, true);
                s += "\"x\":0}";
                break;
            }
        }
    }
};
}  // namespace

// in front of a launch that covers op[0 .. n_ops): describe it and copy what it reads and what it will write.  cp: this pass's copy of
// op[0].conv (the folded upsample lives there), null for the ops that are no convolution
int record_before(LaunchRecorder* r, vc_engine* e, const Op* op, int n_ops, int cfg, const ConvP* cp, bool u8_src, bool side, hipStream_t s) {
    r->launches.push_back(RecLaunch{r->net_id, (int)(op - r->ops0), n_ops, cfg, side ? 1 : 0, "", {}});
    RecLaunch& L = r->launches.back();
    Describe d{e, r, L};
    for (int j = 0; j < n_ops; ++j) {
        if (j) L.ops += ",";
        d.op(L.ops, op[j], j == 0 ? cp : nullptr, j == 0 && u8_src);
    }
    for (RecBuf& b : L.bufs) {
        const size_t sz = (b.bytes + 255) / 256 * 256;
        VC_CHECK(r->used + (b.written ? 2 : 1) * sz <= r->cap, VC_ERR_CAPACITY, "launch recorder: arena of %zu bytes is too small", r->cap);
        b.before = r->used; r->used += sz;
        if (b.written) { b.after = r->used; r->used += sz; }
        VC_HIP(hipMemcpyAsync(r->d_arena + b.before, b.ptr, b.bytes, hipMemcpyDeviceToDevice, s));
    }
    return VC_OK;
}

int record_after(LaunchRecorder* r, hipStream_t s) {
    for (const RecBuf& b : r->launches.back().bufs)
        if (b.written) VC_HIP(hipMemcpyAsync(r->d_arena + b.after, b.ptr, b.bytes, hipMemcpyDeviceToDevice, s));
    return VC_OK;
}

}  // namespace vc

using namespace vc;

extern "C" {

int vc_record_arm(vc_engine* e, int net) {
    VC_CHECK(e, VC_ERR_ARG, "null engine");
    VC_CHECK(net == VC_NET_YOLO || net == VC_NET_REID, VC_ERR_ARG, "bad net id %d", net);
    VC_CHECK(e->finalized && (net == VC_NET_YOLO ? e->cfg.with_detector : e->cfg.with_reid), VC_ERR_STATE, "that network is not finalized");
    e->rec_armed = net + 1;
    return VC_OK;
}

int vc_record_list(vc_engine* e, char* buf, size_t cap, size_t* size) {
    VC_CHECK(e && size, VC_ERR_ARG, "null argument");
    VC_CHECK(e->rec, VC_ERR_STATE, "no recorded pass: vc_record_arm, then run the network");
    const LaunchRecorder* r = e->rec;
    std::string t;
    jf(t, "{\"arena_bytes\":%zu,\"launches\":[", r->used);
    for (size_t i = 0; i < r->launches.size(); ++i) {
        const RecLaunch& L = r->launches[i];
        if (i) t += ",";
        jf(t, "\n{\"net\":%d,\"op0\":%d,\"n_ops\":%d,\"cfg\":%d,\"side\":%d,\"ops\":[", L.net, L.op0, L.n_ops, L.cfg, L.side);
        t += L.ops;
        t += "],\"bufs\":[";
        for (size_t j = 0; j < L.bufs.size(); ++j) {
            const RecBuf& b = L.bufs[j];
            jf(t, "%s{\"name\":\"%s\",\"es\":%d,\"cs\":%d,\"bytes\":%zu,\"written\":%d,\"before\":%zu,\"after\":%zu}", j ? "," : "", b.name.c_str(), b.es, b.cs, b.bytes,
               b.written ? 1 : 0, b.before, b.after);
        }
        t += "]}";
    }
    t += "]}";
    *size = t.size() + 1;
    if (!buf) return VC_OK;
    VC_CHECK(cap >= t.size() + 1, VC_ERR_CAPACITY, "vc_record_list: %zu bytes needed", t.size() + 1);
    memcpy(buf, t.c_str(), t.size() + 1);
    return VC_OK;
}

int vc_record_read(vc_engine* e, void* out, size_t cap) {
    VC_CHECK(e && out, VC_ERR_ARG, "null argument");
    VC_CHECK(e->rec, VC_ERR_STATE, "no recorded pass: vc_record_arm, then run the network");
    VC_CHECK(cap >= e->rec->used, VC_ERR_CAPACITY, "vc_record_read: %zu bytes needed", e->rec->used);
    VC_HIP(hipSetDevice(e->cfg.device));
    VC_HIP(hipStreamSynchronize(e->dstream));
    VC_HIP(hipStreamSynchronize(e->hstream));
    VC_HIP(hipStreamSynchronize(e->rstream));
    VC_HIP(hipStreamSynchronize(e->stream));
    if (e->rec->used) VC_HIP(hipMemcpy(out, e->rec->d_arena, e->rec->used, hipMemcpyDeviceToHost));
    return VC_OK;
}

}  // extern "C"
