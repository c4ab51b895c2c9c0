/* sa_locate.h -- what sa_locate.c (the host build of the reference index) and sa_locate.hip (its device copy, the kernel) share */
#ifndef SA_LOCATE_H
#define SA_LOCATE_H

#include <stdint.h>

#include "signalalign_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SA_LOCATE_K 15

struct sa_ref_index {
    int64_t n_contigs, total, n_entries;
    int32_t q, device;
    char **names;
    int64_t *starts;      /* n_contigs + 1 */
    uint32_t *codes;      /* n_entries, sorted */
    int32_t *pos;         /* n_entries, ascending inside a code */
    int32_t *table;       /* 2^q + 1 */
    double build_seconds;
    /* the device copy (sa_locate.hip); starts as int32: the total is below 2^31 */
    void *d_codes, *d_pos, *d_table, *d_starts;
    int64_t device_bytes;
};

/* sa_locate.hip: the four arrays to idx->device / back to the allocator */
int sa_locate_upload(struct sa_ref_index *idx);
void sa_locate_drop_device(struct sa_ref_index *idx);

#ifdef __cplusplus
}
#endif
#endif
