// api_model.hip — the C ABI (include/gsr.h) of the model files (modelio.hip): the rows of
// point_cloud.ply packed from and unpacked into the ten stored tensors.  Host orchestration only.
#include <stdio.h>

#include "gsr_api_common.h"

using namespace gsr;

static const char* const kTensorNames[10] = {"xyz",      "features_dc", "features_rest", "opacity",  "scaling",
                                             "rotation", "sg_axis",     "sg_sharpness",  "sg_color", "filter_3D"};

// `who`: P >= 0, the degrees in range, every tensor that has a column present; *A receives the row length
static int check_model(const char* who, long long P, int M, int G, const float* const* t, int* A) {
    char msg[128];
    if (P < 0) return snprintf(msg, sizeof msg, "%s: `P` is negative", who), fail(GSR_ERR_ARGS, msg);
    *A = model_row_floats(M, G);
    if (*A == 0)
        return snprintf(msg, sizeof msg, "%s: `M` must be in [1, 2^20] and `G` in [0, 2^20]", who), fail(GSR_ERR_ARGS, msg);
    if (model_block_rows(*A) == 0)
        return snprintf(msg, sizeof msg, "%s: a row of %d floats does not fit a workgroup's tile", who, *A),
               fail(GSR_ERR_ARGS, msg);
    if (P == 0) return GSR_OK;
    const bool need[10] = {true, true, M > 1, true, true, true, G > 0, G > 0, G > 0, true};
    for (int k = 0; k < 10; k++)
        if (need[k] && !t[k])
            return snprintf(msg, sizeof msg, "%s: missing buffer `%s`", who, kTensorNames[k]), fail(GSR_ERR_ARGS, msg);
    return GSR_OK;
}

extern "C" {

int gsr_model_row_floats(int M, int G) { return model_row_floats(M, G); }

int gsr_model_block_rows(int A) { return model_block_rows(A); }

int gsr_model_unpack_block_rows(long long stride) { return model_unpack_block_rows(stride); }

int gsr_model_pack_rows(long long P, int M, int G, const float* xyz, const float* features_dc,
                        const float* features_rest, const float* opacity, const float* scaling, const float* rotation,
                        const float* sg_axis, const float* sg_sharpness, const float* sg_color, const float* filter_3D,
                        float* rows, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    const float* t[10] = {xyz,      features_dc, features_rest, opacity,  scaling,
                          rotation, sg_axis,     sg_sharpness,  sg_color, filter_3D};
    int A = 0;
    if (int rc = check_model("model_pack_rows", P, M, G, t, &A)) return rc;
    if (P == 0) return GSR_OK;
    if (!rows) return fail(GSR_ERR_ARGS, "model_pack_rows: missing buffer `rows`");
    if ((P + model_block_rows(A) - 1) / model_block_rows(A) >= 2147483648LL)
        return fail(GSR_ERR_ARGS, "model_pack_rows: 2^31 or more workgroups");
    GSR_CHECK(launch_model_pack_rows(P, M, G, t, rows, stream), "model pack rows");
    return GSR_OK;
}

int gsr_model_unpack_rows(long long P, int M, int G, long long stride, const uint8_t* rows, const int32_t* col_offset,
                          const int32_t* col_type, float* xyz, float* features_dc, float* features_rest,
                          float* opacity, float* scaling, float* rotation, float* sg_axis, float* sg_sharpness,
                          float* sg_color, float* filter_3D, void* stream_ptr) {
    hipStream_t stream = (hipStream_t)stream_ptr;
    float* t[10] = {xyz, features_dc, features_rest, opacity, scaling, rotation, sg_axis, sg_sharpness, sg_color, filter_3D};
    int A = 0;
    if (int rc = check_model("model_unpack_rows", P, M, G, t, &A)) return rc;
    if (stride < 1) return fail(GSR_ERR_ARGS, "model_unpack_rows: `stride` must be positive");
    const int R = model_unpack_block_rows(stride);
    if (R == 0) return fail(GSR_ERR_ARGS, "model_unpack_rows: a row of `stride` bytes does not fit a workgroup's tile");
    if (P == 0) return GSR_OK;
    if (!rows || !col_offset || !col_type) return fail(GSR_ERR_ARGS, "model_unpack_rows: missing buffer");
    if (reinterpret_cast<uintptr_t>(rows) & 15u)
        return fail(GSR_ERR_ARGS, "model_unpack_rows: `rows` must be 16-byte aligned");
    if ((P + R - 1) / R >= 2147483648LL) return fail(GSR_ERR_ARGS, "model_unpack_rows: 2^31 or more workgroups");
    // The column tables are checked on the host before the launch (a column past the end of its row
    // would be read from the next row, or from outside the staged bytes): 8 A bytes come back, and
    // the call waits for them.  The file system, not this wait, is what a load spends its time in.
    std::vector<int32_t> table(2 * (size_t)A);
    GSR_CHECK(hipMemcpyAsync(table.data(), col_offset, (size_t)A * 4, hipMemcpyDeviceToHost, stream), "column table");
    GSR_CHECK(hipMemcpyAsync(table.data() + A, col_type, (size_t)A * 4, hipMemcpyDeviceToHost, stream), "column table");
    GSR_CHECK(hipStreamSynchronize(stream), "column table");
    for (int c = 0; c < A; c++) {
        if (c >= 3 && c < 6) continue;  // (nx ny nz: no tensor reads them)
        const int32_t off = table[c], type = table[A + c];
        if (off < -1) return fail(GSR_ERR_ARGS, "model_unpack_rows: a column offset below -1");
        if (off < 0) continue;
        if (type != 0 && type != 1) return fail(GSR_ERR_ARGS, "model_unpack_rows: a column type other than 0 or 1");
        if ((long long)off + (type ? 8 : 4) > stride)
            return fail(GSR_ERR_ARGS, "model_unpack_rows: a column ends past `stride`");
    }
    GSR_CHECK(launch_model_unpack_rows(P, M, G, stride, rows, col_offset, col_type, t, stream), "model unpack rows");
    return GSR_OK;
}

}  // extern "C"
