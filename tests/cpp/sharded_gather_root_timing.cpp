// sharded_gather_root_timing.cpp -- clm4_sharded_gemm_enqueue in mode CLM4_GEMM_GATHER_ROOT with eight shards on ONE device: the events of
// a timed step are ordered kernel begin <= kernel end <= exchange end on EVERY shard, also on the shards that exchange nothing, and also
// when the compute streams are far behind the host.  BACKLOG untimed steps are enqueued without a wait, then one timed step; every
// shard's clm4_sharded_step_timing must give kernel > 0 and exchange >= 0.  Prints "shard p kernel_ms exchange_ms" and "timing ok" /
// "timing FAILED"; "no_device" without a GPU.
#include <clover_hip.h>

#include <cstdio>

#define CHECK(call)                                                                       \
    do {                                                                                  \
        int rc__ = (call);                                                                \
        if (rc__ != CLV_OK) {                                                             \
            std::printf("FAILED %s -> %d: %s\n", #call, rc__, clv_last_error());          \
            return 1;                                                                     \
        }                                                                                 \
    } while (0)

int main()
{
    int ndev = 0;
    CHECK(clv_device_count(&ndev));
    if (ndev == 0) { std::printf("no_device\n"); return 0; }
    CHECK(clv_set_device(0));
    const uint64_t rows = 8192, K = 4096, N = 2048;      // N: kernels long enough for the compute streams to fall behind the host
    const int parts = 8, BACKLOG = 20;
    const int zeros[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    clm4_shard_ctx *ctx = nullptr;
    CHECK(clm4_sharded_create(&ctx, parts, zeros, rows, K));
    CHECK(clm4_sharded_fill_random(ctx, 7));
    int8_t *B; float *sB;
    CHECK(clv_malloc((void **)&B, N * K / 2));
    CHECK(clv_malloc((void **)&sB, (N / 64) * (K / 64) * 4));
    CHECK(clv_fill_random_nibbles(B, N * K / 2, 8, 0, nullptr));
    CHECK(clv_fill_random_scales(sB, (N / 64) * (K / 64), 9, 0, nullptr));
    CHECK(clv_device_sync());
    int bad = 0;
    for (int round = 0; round < 3; round++) {
        CHECK(clm4_sharded_gemm_begin_mode(ctx, B, sB, N, 0, 1, CLM4_GEMM_GATHER_ROOT));
        for (int step = 1; step <= BACKLOG; step++) CHECK(clm4_sharded_gemm_enqueue(ctx, step, 0));
        CHECK(clm4_sharded_gemm_enqueue(ctx, 0, 1));
        CHECK(clm4_sharded_sync(ctx));
        for (int p = 0; p < parts; p++) {
            float k = -1.0f, g = -1.0f;
            CHECK(clm4_sharded_step_timing(ctx, p, 0, &k, &g));
            std::printf("round %d shard %d kernel_ms=%.4f exchange_ms=%.4f\n", round, p, k, g);
            if (!(k > 0.0f) || !(g >= 0.0f)) bad++;
        }
    }
    CHECK(clv_free(B)); CHECK(clv_free(sB));
    CHECK(clm4_sharded_destroy(ctx));
    std::printf(bad ? "timing FAILED (%d)\n" : "timing ok\n", bad);
    return bad ? 1 : 0;
}
