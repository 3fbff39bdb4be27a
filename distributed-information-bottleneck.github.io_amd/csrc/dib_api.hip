// dib_api.hip - the one translation unit of libdib_hip.so, the C ABI (include/*.h) of the MI355X Distributed-IB hot path: the
// kernel headers (dib_*.h) and, below them, the host code by family (host/*.h).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/dib_hip.h"
#include "dib_elementwise.h"
#include "dib_gauss_lse.h"
#include "dib_mi_rows.h"
#include "dib_gemm.h"
#include "dib_gemm_stream.h"
#include "dib_wgrad_stream.h"
#include "dib_infonce_mfma.h"
#include "dib_fused.h"
#include "dib_wgrad_recompute.h"
#include "dib_tail.h"
#include "dib_small.h"
#include "dib_st.h"
#include "dib_attn.h"
#include "dib_attn_small.h"
#include "dib_st_chain.h"
#include "dib_measure.h"
#include "dib_circuit.h"
#include "dib_partition.h"
#include "dib_st_info.h"
#include "dib_mi_channel.h"
#include "dib_input_grad.h"
#include "../../include/dib_st.h"
#include "../../include/dib_measure.h"
#include "../../include/dib_circuit.h"
#include "../../include/dib_partition.h"
#include "../../include/dib_mi_channel.h"

// The host code, by family, in dependency order (this file is the only translation unit).
#include "host/common.h"
#include "host/layout.h"
#include "host/gemm.h"
#include "host/encoder.h"
#include "host/input_grad.h"
#include "host/small.h"
#include "host/step.h"
#include "host/infonce.h"
#include "host/st.h"
#include "host/mi.h"
#include "host/measure.h"
#include "host/circuit.h"
#include "host/partition.h"
