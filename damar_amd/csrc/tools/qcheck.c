/* qcheck -- host/quality.c and the traces-on reader of host/piles.c as a program of their own, without the GPU runtime and
 * without the library: the annotate pass of LAq over a .las file on the host path, the tracks written and read back, then
 * the -u pass.  It exists to run that code under sanitizers, which a library loaded into Python does not allow:
 *
 *   gcc -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude -Idamar_amd/csrc -Idamar_amd/csrc/host \
 *       -o qcheck damar_amd/csrc/tools/qcheck.c damar_amd/csrc/host/quality.c damar_amd/csrc/host/piles.c damar_amd/csrc/host/db.c -lz -lm
 *   (cd <directory of the database>; qcheck G file.las [segmin segmax])      # DAMAR_PILE_BATCH / DAMAR_PILE_TRACE_BYTES cut batches
 *
 * It writes the tracks "sq" and "st" beside the database.  damar_pile_quality, the shim's in the library, is the host path here. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "damar_hip.h"
#include "damar_host.h"
int damar_pile_quality(const damar_trace_batch *t, const damar_q_params *p, int *q, int64 *nt)
{ if (!damar_trace_batch_valid(t, nt)) return 1;
  if (q == NULL || *nt == 0) return 0;
  return damar_host_pile_quality(t, p, q);
}
int main(int argc, char **argv)
{ damar_dbinfo db; damar_q_params p = { 1, 20, 0 }; damar_q_result res, upd; int rc;
  uint64 *qa, *ta; int *qd, *td; int64 nq, nt;
  if (argc < 3 || damar_dbinfo_open(argv[1], &db)) return 2;
  if (argc > 3) { p.segmin = atoi(argv[3]); p.segmax = atoi(argv[4]); }
  rc = damar_q_track(&db, argv[2], &p, 25, 1000, &res);
  if (rc == 0)
    { unsigned long long h = 0; int64 i;
      for (i = 0; i < res.nq; i++) h = h * 1000003ull + (unsigned) res.q_data[i];
      for (i = 0; i < res.ntrim; i++) h = h * 1000003ull + (unsigned) res.trim_data[i];
      printf("nq %lld ntrim %lld hash %llx\n", (long long) res.nq, (long long) res.ntrim, h);
      damar_track_write_a2(db.path, "sq", 0, db.nreads, res.q_anno, res.q_data, res.nq);
      damar_track_write_a2(db.path, "st", 0, db.nreads, res.trim_anno, res.trim_data, res.ntrim);
      if (damar_track_read_a2(db.path, "sq", db.nreads, &qa, &qd, &nq) || damar_track_read_a2(db.path, "st", db.nreads, &ta, &td, &nt)) return 3;
      if (nq != res.nq || memcmp(qd, res.q_data, 4 * nq) || nt != res.ntrim) return 4;
      rc = damar_trim_update(&db, argv[2], qa, qd, nq, ta, td, 25, 1000, 0, &upd);
      printf("update rc %d ntrim %lld\n", rc, (long long) upd.ntrim);
      damar_q_result_free(&upd);
      free(qa); free(qd); free(ta); free(td);
    }
  damar_q_result_free(&res);
  damar_dbinfo_close(&db);
  return rc;
}
