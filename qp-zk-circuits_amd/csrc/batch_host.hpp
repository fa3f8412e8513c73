// batch_host.hpp — shared by the host code of the aggregation levels (batch.cpp, proof_targets.cpp).
#pragma once

namespace batch {
// the reason (printf form) into the caller's QPGPU_BATCH_ERR_CAP bytes, where there are any; returns `code`
int fail(char *err, int code, const char *fmt, ...);
}
