// Inverted ("CSR") index of a scatter, built per cloud, and the scatter-add backward that runs through it.
// idx (B, ne) names a target in [0, m) per entry; list(k) = the entries with idx == k, start (B, m + 1) their bounds.
// Entries outside [0, m) are in no list.  The order inside a list comes from an LDS atomic cursor: it is not fixed
// between launches.  Users: three_interpolate and its rows form (interpolate.hip), group_points and the channels-last
// QueryAndGroup (group_points.hip).
#pragma once
#include "common.h"

namespace pdm {

enum CsrPayload {
    CSR_ROW_WEIGHT,   // an entry holds (source row = e / per as 16 bits, weight[e] or 1 without weights)
    CSR_ELEMENT       // an entry holds its own number e
};

struct CsrLists {            // cloud b: start + b * (m + 1), the payload arrays + b * ne
    int *start;
    unsigned short *row;     // CSR_ROW_WEIGHT
    float *weight;           // CSR_ROW_WEIGHT
    int *elem;               // CSR_ELEMENT
};

constexpr int CSR_MAX_TARGETS = 16384;   // the histogram of a cloud lives in LDS

size_t csr_workspace_bytes(CsrPayload payload, int b, long long ne, int m);
// the sections of a workspace of csr_workspace_bytes (8-byte aligned or better)
CsrLists csr_carve(void *workspace, CsrPayload payload, int b, long long ne, int m);
// one workgroup per cloud: count -> scan -> fill.  m <= CSR_MAX_TARGETS; weight may be null; returns check_launch(who)
int csr_build_launch(void *stream, const char *who, CsrPayload payload, int b, int ne, int per, int m, const int *idx,
                     const float *weight, const CsrLists &lists);

// grad_points[b, c, k] += sum over list(k) of weight * grad_out[b, c, row]: rows of `row_len` floats per (cloud, channel),
// ne = per * row_len entries per cloud.  Workspace: csr_workspace_bytes(CSR_ROW_WEIGHT, b, ne, m).
bool csr_form_applies(int b, int row_len, long long ne, int m);
int csr_scatter_grad_launch(void *stream, const char *who, int b, int c, int row_len, int per, int m, const float *grad_out,
                            const int *idx, const float *weight, float *grad_points, void *workspace);

}  // namespace pdm
