// The text tower's entry points of the C ABI (include/revo.h, TEXT: revo_text_create, revo_text_forward, revo_text_destroy,
// revo_op_attention_causal, revo_op_embed_tokens, revo_op_pool_eot) under AddressSanitizer + UBSan: every refusal they make
// before the device is touched, with its message; the host arrays they are given are exactly as long as the call says.  Needs no GPU: without one
// a complete checkpoint gets as far as the device and fails there with -1, which is checked too.  Where a device is present
// the refusals that need a live handle (batch above max_batch, seq_len above the context, a bad token id) run as well.
// Built by `make -C revers-o_amd/csrc text_check` and run by tests/test_text_host.py in the CPU tier.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/revo.h"

static int failures = 0;
static void section(const char* name) { std::printf("case: %s\n", name); }
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d  %s   [last error: %s]\n", __FILE__, __LINE__, #cond, revo_last_error()); ++failures; } \
    } while (0)
static bool err_has(const char* needle) { return std::strstr(revo_last_error(), needle) != nullptr; }

struct Checkpoint {
    std::vector<std::string> names;
    std::vector<std::vector<float>> data;
    std::vector<revo_tensor> t;
    void add(const std::string& n, int64_t numel) { names.push_back(n); data.emplace_back((size_t)numel, 0.01f); }
    void finish() {
        t.clear();
        for (size_t i = 0; i < names.size(); ++i) t.push_back({names[i].c_str(), data[i].data(), (int64_t)data[i].size()});
    }
    void drop(const std::string& n) {
        for (size_t i = 0; i < names.size(); ++i)
            if (names[i] == n) { names.erase(names.begin() + i); data.erase(data.begin() + i); break; }
        finish();
    }
};
static Checkpoint make(const revo_text_cfg& c) {
    Checkpoint k;
    const int64_t W = c.width, M = c.mlp_dim;
    k.add("token_embedding.weight", (int64_t)c.vocab_size * W);
    k.add("positional_embedding", (int64_t)c.context_length * W);
    k.add("ln_final.weight", W); k.add("ln_final.bias", W);
    k.add("text_projection", W * c.out_dim);
    for (int i = 0; i < c.layers; ++i) {
        const std::string p = "transformer.resblocks." + std::to_string(i) + ".";
        for (const char* n : {"ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "attn.out_proj.bias", "mlp.c_proj.bias"}) k.add(p + n, W);
        k.add(p + "attn.in_proj_weight", 3 * W * W); k.add(p + "attn.in_proj_bias", 3 * W);
        k.add(p + "attn.out_proj.weight", W * W);
        k.add(p + "mlp.c_fc.weight", M * W); k.add(p + "mlp.c_fc.bias", M);
        k.add(p + "mlp.c_proj.weight", W * M);
        if (c.use_ls) { k.add(p + "ls_1.gamma", W); k.add(p + "ls_2.gamma", W); }
    }
    k.finish();
    return k;
}

int main() {
    const revo_text_cfg good = {16, 64, 128, 2, 2, 512, 64, 0, 1e-5f};
    Checkpoint ck = make(good);
    revo_text* h = nullptr;
    std::vector<int32_t> tok(3 * 5, 1);
    std::vector<float> out(3 * 64);

    section("create: null arguments");
    EXPECT(revo_text_create(nullptr, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("null argument"));
    EXPECT(revo_text_create(&good, nullptr, 0, 0, 4, &h) == -2 && err_has("null argument"));
    EXPECT(revo_text_create(&good, ck.t.data(), (int)ck.t.size(), 0, 4, nullptr) == -2 && err_has("null argument"));
    EXPECT(revo_text_create(&good, ck.t.data(), (int)ck.t.size(), 0, 0, &h) == -2 && err_has("max_batch"));

    section("create: shapes the kernels do not take");
    {
        revo_text_cfg c = good; c.heads = 4;                 // head_dim 32
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("head_dim must be 64"));
        c = good; c.heads = 0;
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("positive"));
        c = good; c.context_length = 129;
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("context_length above 128"));
        c = good; c.width = 96; c.heads = 1;                 // head_dim 96
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("head_dim must be 64"));
        c = good; c.mlp_dim = 500;
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("multiples of 64"));
        c = good; c.out_dim = 62;
        EXPECT(revo_text_create(&c, ck.t.data(), (int)ck.t.size(), 0, 4, &h) == -2 && err_has("out_dim"));
    }

    section("create: the checkpoint, by name");
    {
        Checkpoint k = make(good);
        k.drop("transformer.resblocks.1.mlp.c_fc.bias");
        EXPECT(revo_text_create(&good, k.t.data(), (int)k.t.size(), 0, 4, &h) == -2 &&
               err_has("missing weight tensor: transformer.resblocks.1.mlp.c_fc.bias"));
        k = make(good);
        k.add("visual.proj", 8); k.finish();
        EXPECT(revo_text_create(&good, k.t.data(), (int)k.t.size(), 0, 4, &h) == -2 && err_has("unexpected weight tensor: visual.proj"));
        revo_text_cfg ls = good; ls.use_ls = 1;
        k = make(ls);
        EXPECT(revo_text_create(&good, k.t.data(), (int)k.t.size(), 0, 4, &h) == -2 && err_has("LayerScale needs cfg.use_ls = 1"));
        revo_text_cfg wide = good; wide.vocab_size = 65;     // the table of a 64-word vocabulary is one row short
        k = make(good);
        EXPECT(revo_text_create(&wide, k.t.data(), (int)k.t.size(), 0, 4, &h) == -2 && err_has("weight token_embedding.weight: expected"));
        k = make(good);
        k.t[0].data = nullptr;
        EXPECT(revo_text_create(&good, k.t.data(), (int)k.t.size(), 0, 4, &h) == -2 && err_has("null name or data"));
    }

    section("forward: refusals that need no handle");
    EXPECT(revo_text_forward(nullptr, tok.data(), 0, 5, out.data(), 1, nullptr) == -2 && err_has("at least 1"));
    EXPECT(revo_text_forward(nullptr, tok.data(), -3, 5, out.data(), 1, nullptr) == -2 && err_has("at least 1"));
    EXPECT(revo_text_forward(nullptr, tok.data(), 3, 0, out.data(), 1, nullptr) == -2 && err_has("at least 1"));
    EXPECT(revo_text_forward(nullptr, tok.data(), 3, 5, out.data(), 1, nullptr) == -2 && err_has("null argument"));
    EXPECT(revo_text_destroy(nullptr) == 0);

    section("ops: refusals");
    {
        std::vector<uint16_t> qkv(8 * 192 + 64), o(8 * 64 + 64);
        EXPECT(revo_op_attention_causal(qkv.data(), 192, o.data(), 64, 1, 8, 1, 96, nullptr) == -2 && err_has("head_dim must be 64"));
        EXPECT(revo_op_attention_causal(qkv.data(), 192, o.data(), 64, 1, 129, 1, 64, nullptr) == -2 && err_has("128"));
        EXPECT(revo_op_attention_causal(qkv.data(), 196, o.data(), 64, 1, 8, 1, 64, nullptr) == -2 && err_has("strides"));
        EXPECT(revo_op_attention_causal(qkv.data(), 192, o.data(), 66, 1, 8, 1, 64, nullptr) == -2 && err_has("strides"));
        EXPECT(revo_op_attention_causal(qkv.data(), 128, o.data(), 64, 1, 8, 1, 64, nullptr) == -2 && err_has("strides"));
        EXPECT(revo_op_attention_causal(nullptr, 192, o.data(), 64, 1, 8, 1, 64, nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_op_attention_causal(qkv.data(), 192, o.data(), 64, -1, 8, 1, 64, nullptr) == -2 && err_has("negative"));
        EXPECT(revo_op_attention_causal(qkv.data(), 192, o.data(), 64, 0, 8, 1, 64, nullptr) == 0);
        std::vector<float> tab(64 * 8), x(64);
        EXPECT(revo_op_embed_tokens(nullptr, tab.data(), tab.data(), 1, 1, 64, 8, x.data(), 8, nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_op_embed_tokens(tok.data(), tab.data(), tab.data(), 1, 0, 64, 8, x.data(), 8, nullptr) == -2);
        EXPECT(revo_op_embed_tokens(tok.data(), tab.data(), tab.data(), 1, 1, 64, 6, x.data(), 8, nullptr) == -2 && err_has("multiples of 4"));
        EXPECT(revo_op_embed_tokens(tok.data(), tab.data(), tab.data(), 1, 1, 64, 8, x.data(), 4, nullptr) == -2);
        EXPECT(revo_op_embed_tokens(tok.data(), tab.data(), tab.data(), 1, 1, 0, 8, x.data(), 8, nullptr) == -2);
        EXPECT(revo_op_embed_tokens(tok.data(), tab.data(), tab.data(), 0, 1, 64, 8, x.data(), 8, nullptr) == 0);
        EXPECT(revo_op_pool_eot(nullptr, tab.data(), 8, 1, 1, 8, x.data(), nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_op_pool_eot(tok.data(), nullptr, 8, 1, 1, 8, x.data(), nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 8, 1, 1, 8, nullptr, nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 8, 1, 0, 8, x.data(), nullptr) == -2 && err_has("bad batch or seq"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 8, -1, 1, 8, x.data(), nullptr) == -2 && err_has("bad batch or seq"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 4, 1, 1, 8, x.data(), nullptr) == -2 && err_has("row stride below width"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 8, 1, 1, 6, x.data(), nullptr) == -2 && err_has("multiples of 4"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 10, 1, 1, 8, x.data(), nullptr) == -2 && err_has("multiples of 4"));
        EXPECT(revo_op_pool_eot(tok.data(), tab.data(), 8, 0, 1, 8, x.data(), nullptr) == 0);
    }

    section("create: a complete checkpoint reaches the device");
    const int rc = revo_text_create(&good, ck.t.data(), (int)ck.t.size(), 0, 3, &h);
    EXPECT(rc == 0 || rc == -1);                              // -1: no device here; nothing was validated away
    if (rc == 0) {
        section("forward: refusals on a live handle");
        EXPECT(revo_text_forward(h, tok.data(), 4, 3, out.data(), 1, nullptr) == -2 && err_has("max_batch"));
        EXPECT(revo_text_forward(h, tok.data(), 1, 17, out.data(), 1, nullptr) == -2 && err_has("context_length"));
        EXPECT(revo_text_forward(h, nullptr, 3, 5, out.data(), 1, nullptr) == -2 && err_has("null argument"));
        EXPECT(revo_text_forward(h, tok.data(), 3, 5, nullptr, 1, nullptr) == -2 && err_has("null argument"));
        tok[2 * 5 + 3] = 64;
        EXPECT(revo_text_forward(h, tok.data(), 3, 5, out.data(), 1, nullptr) == -2 && err_has("prompt 2 position 3 holds token id 64"));
        tok[2 * 5 + 3] = -1;
        EXPECT(revo_text_forward(h, tok.data(), 3, 5, out.data(), 1, nullptr) == -2 && err_has("prompt 2 position 3 holds token id -1"));
        EXPECT(revo_text_destroy(h) == 0);
    } else {
        std::printf("no device: the live-handle refusals are left to the GPU tier\n");
    }

    if (failures) { std::printf("%d FAILED\n", failures); return 1; }
    std::printf("ALL OK\n");
    return 0;
}
