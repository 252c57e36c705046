/* oracle/ref_repeater/freedv_api_internal.h -- ours: the two status bits tx/frame_repeater.c reads, for oracle/build_ref_repeater.sh */
#include <stdint.h>
#include <string.h>
#define FREEDV_RX_SYNC 0x2 /* [UPSTREAM-RECALLED codec2 src/freedv_api.h] */
#define FREEDV_RX_BITS 0x4 /* [UPSTREAM-RECALLED codec2 src/freedv_api.h] */
