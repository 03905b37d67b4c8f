/* stitch_host.c -- the host path of LAstitch as a program of its own, without the GPU library: host/stitch.c and
 * host/bridge.c around a damar_trace_boxes that is the host routine and nothing else.  For runs of the host code under
 * a sanitizer on the CPU (the library itself is never loaded into one):
 *
 *   gcc -g -O1 -fsanitize=address,undefined -Iinclude -Idamar_amd/csrc -o stitch_host damar_amd/csrc/tools/stitch_host.c \
 *       damar_amd/csrc/host/{stitch,bridge,piles,quality,db}.c -lm -lz -lpthread
 *   ./stitch_host [-p] [-f <int>] [-t <track>] <db> <in.las> <out.las>
 *
 * The calls of the device paths that piles.c and quality.c refer to are never reached from here and end the program. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "host/damar_host.h"

int damar_trace_boxes(const damar_tbox_batch *b, int *diffs, int64 *toff, uint16 **trace)
{ int64 i;
  int   tlen;
  toff[0] = 0;
  for (i = 0; i < b->nbox; i++)
    toff[i + 1] = toff[i] + 2 * (int64) ((b->abpos[i] % b->tspace + b->m[i] + b->tspace - 1) / b->tspace);
  if ((*trace = (uint16 *) malloc(sizeof(uint16) * (size_t) toff[b->nbox] + 8)) == NULL)
    return 1;
  for (i = 0; i < b->nbox; i++)
    { diffs[i] = damar_trace_box(b->bases + b->aoff[i], b->m[i], b->bases + b->boff[i], b->n[i], b->abpos[i], b->tspace, *trace + toff[i], &tlen);
      if (tlen != toff[i + 1] - toff[i])
        return 1;
    }
  return 0;
}

int64 damar_stat_bridges;              /* redundancy.c's counter of daligner's own bridging, which bridge.c adds to */

static void not_here(const char *what)
{ fprintf(stderr, "stitch_host: %s is a call of the GPU library\n", what);
  exit(2);
}

int  damar_pile_quality(const damar_trace_batch *b, const damar_q_params *p, int *q_out, int64 *ntiles_out)
{ (void) b; (void) p; (void) q_out; (void) ntiles_out; not_here("damar_pile_quality"); return 1; }
int  damar_pile_coverage(const damar_pile_batch *b, const damar_repeat_params *p, int64 *histo, int64 *bases, int64 *inactive)
{ (void) b; (void) p; (void) histo; (void) bases; (void) inactive; not_here("damar_pile_coverage"); return 1; }
int  damar_pile_repeats(const damar_pile_batch *b, const damar_repeat_params *p, damar_pile_track *out)
{ (void) b; (void) p; (void) out; not_here("damar_pile_repeats"); return 1; }
int  damar_pile_tandem(const damar_pile_batch *b, int min_len, damar_pile_track *out)
{ (void) b; (void) min_len; (void) out; not_here("damar_pile_tandem"); return 1; }

int main(int argc, char *argv[])
{ damar_stitch_params p;
  damar_stitch_stats  st;
  int c;
  memset(&p, 0, sizeof(p));
  p.fuzz = 40;  p.anchor = 500;  p.merge = 10;  p.min_len = 500;  p.min_merge = 200;  p.gap_diff = 0.3;
  while ((c = getopt(argc, argv, "pf:t:")) != -1)
    switch (c)
      { case 'p': p.purge = 1; break;
        case 'f': p.fuzz = atoi(optarg); break;
        case 't': p.lc_track = optarg; break;
        default: return 1;
      }
  if (argc - optind != 3)
    { fprintf(stderr, "usage: stitch_host [-p] [-f <int>] [-t <track>] <db> <in.las> <out.las>\n");
      return 1;
    }
  if (damar_stitch_las(argv[optind], argv[optind + 1], argv[optind + 2], &p, &st))
    return 1;
  damar_bridge_release();
  printf("stitched %lld (low complexity %lld) out of %lld, %lld boxes (%lld widened) in %lld rounds, %lld refused, %lld without a box\n",
         (long long) st.stitched, (long long) st.stitched_lc, (long long) st.novl, (long long) st.boxes, (long long) st.widened,
         (long long) st.rounds, (long long) st.refused, (long long) st.no_box);
  return 0;
}
