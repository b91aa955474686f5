// run_bytes.h — how many bytes the run of one kept record holds, by record type.  The per-record byte runs (the names behind
// inq_read_origin_t, the packed bases behind inq_read_seq_t) lie back to back in their records' order: the device scans these lengths
// (bam_scan.hip), the host driver cuts the fetched bytes by them (driver_internal.h).  A further payload is one more overload.
#pragma once
#include <stdint.h>

#include "../../include/inquistr_hip.h"

#ifdef __HIPCC__
#define INQ_HOST_DEVICE __host__ __device__
#else
#define INQ_HOST_DEVICE
#endif

namespace inq {
INQ_HOST_DEVICE inline uint64_t run_bytes(const inq_read_origin_t &o) { return o.name_len; }
INQ_HOST_DEVICE inline uint64_t run_bytes(const inq_read_seq_t &q) { return ((uint64_t)q.n_bases + 1u) / 2u; }
}  // namespace inq
