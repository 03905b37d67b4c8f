/* LAfilter -- decides which overlaps reach the overlap graph: the command of scrub/LAfilter.c (option letters, usage text,
 * messages and exit codes of its main, :2895-3458) around damar_filter_las (filter.c).  The piles run on the GPU
 * (kernels/pile_filter.hip) unless DAMAR_PILES=host is set; -T trims the overlaps first (trim.c, kernels/box_align.hip
 * unless DAMAR_TRIM=host).
 * -L (the reference's two passes with cached reads) is accepted and changes nothing: all reads are in memory here.
 * A missing trim track is a line on stderr as in the reference, but an error under -T.
 * The reference's experimental options are not supported, each a message and exit status 1: -m -M -y (repeat modules), -P
 * (repeat spanners), -Z (worst alignments), -D -V -W (repeat interval analysis), -c (chimer detection), -j (obsolete). */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "damar_hip.h"
#include "damar_host.h"

static void usage(void)
{ fprintf(stderr, "[-vpLqTwZj] [-dnolRsSumMfyYzZVWb <int>] [-rtD <track>] [-xPIaA <file>] [-c<int,int>] <db> <overlaps_in> <overlaps_out>\n");
  fprintf(stderr, "options: -v ... verbose\n");
  fprintf(stderr, "         -d ... max divergence allowed [0,100]\n");
  fprintf(stderr, "         -n ... min number of non-repeat bases\n");
  fprintf(stderr, "         -o ... min overlap length\n");
  fprintf(stderr, "         -l ... min read length\n");
  fprintf(stderr, "         -p ... purge discarded overlaps\n");
  fprintf(stderr, "         -s ... stitch (%d)\n", -1);
  fprintf(stderr, "         -S ... stitch aggressively (%d)\n", -1);
  fprintf(stderr, "         -r ... repeat track name (%s)\n", "repeats");
  fprintf(stderr, "         -t ... trim track name (%s)\n", "trim");
  fprintf(stderr, "         -T ... trim overlaps (%d)\n", 0);
  fprintf(stderr, "         -u ... max number of unaligned bases\n");
  fprintf(stderr, "         -R ... remove (multiple -R possible) ... \n");
  fprintf(stderr, "                0 stitched overlaps, i.e. overlaps with invalid trace points\n");
  fprintf(stderr, "                1 module overlaps\n");
  fprintf(stderr, "                2 trace points\n");
  fprintf(stderr, "                3 non-identity overlaps\n");
  fprintf(stderr, "                4 remove B-read repeat overlaps, if a proper overlap between A and B exists \n");
  fprintf(stderr, "                5 identity overlaps\n");
  fprintf(stderr, "                6 contained overlaps (includes duplicates)\n");
  fprintf(stderr, "         -L ... two pass processing with read caching\n");
  fprintf(stderr, "experimental features:\n");
  fprintf(stderr, "         -f ... percentage of overlaps to keep (downsampling)\n");
  fprintf(stderr, "         -m ... resolve repeat modules, pass coverage as argument\n");
  fprintf(stderr, "         -M ... -m + more aggressive module detection\n");
  fprintf(stderr, "         -x ... exclude read ids found in file\n");
  fprintf(stderr, "         -I ... include read ids found in file, all other are excluded\n");
  fprintf(stderr, "         -P ... write read ids of repeat spanners to file\n");
  fprintf(stderr, "         -z ... drop entering/leaving alignments if number is below -z <int>\n");
  fprintf(stderr, "         -y ... merge repeats if they are closer then -y bases apart (if distance > 100, then smaller repeats (< 100) usually from DBdust are ignored)\n");
  fprintf(stderr, "         -Y ... merge repeats with start/end position of read if repeat interval starts/ends with fewer then -Y\n");
  fprintf(stderr, "         -a ... write discarded overlaps that may not symmetrically removed to file\n");
  fprintf(stderr, "         -A ... read file of discarded overlaps and remove them symmetrically\n");
  fprintf(stderr, "         -w ... remove multi-mapper overlaps within the same read\n");
  fprintf(stderr, "         -Z ... remove at most -Z percent of the worst alignments. Set -d INT to avoid loss of good alignments. Set -z INT to avoid loss of contiguity !\n");
  fprintf(stderr, "                This option was included to get rid of low coverage repeats or random alignments, that clearly get separated by diff scores\n");
  fprintf(stderr, "         -D ... read low complexity track (dust or tan_dust)\n");
  fprintf(stderr, "         -V ... max merge distance of neighboring repeats (default: 2400)\n");
  fprintf(stderr, "         -W ... window size in bases. Merge repeats that are closer then -V bases and have a decent number of low complexity bases in between both repeats\n");
  fprintf(stderr, "                or at -W bases at the tips of the neighboring repeat. Those can cause a fragmented repeat mask. (default: 600)\n");
  fprintf(stderr, "         -b ... remove alignments which have segments error rates above -b <int>%% (default: not set)\n");
  fprintf(stderr, "         -c <inta,intb> remove overlaps from chimeric reads (Chimer detection: locations that have less then <inta> coverage and less then in <intb> anchor bases around that location)\n");
  fprintf(stderr, "OBSOLETE - will be removed in future\n");
  fprintf(stderr, "         -j ... trim off unaligned bases (indels) from start/end of alignments\n");
}

int main(int argc, char *argv[])
{ damar_filter_opts  o;
  damar_filter_stats st;
  const char *unsupported = NULL;
  int c, rc;

  memset(&o, 0, sizeof(o));
  o.p.seg_rate = -1;  o.p.stitch = -1;
  o.p.min_rlen = o.p.min_olen = o.p.max_unaligned = o.p.min_nonrep = -1;
  o.p.max_diffs = -1;
  o.trim_track = "trim";
  o.rep_track = "repeats";
  opterr = 0;
  while ((c = getopt(argc, argv, "TvLpwy:z:d:n:o:l:R:s:S:u:m:M:r:t:P:x:f:I:Y:a:A:Z:D:V:W:b:jc:")) != -1)
    switch (c)
      { case 'f': o.p.downsample = atoi(optarg); break;
        case 'T': o.do_trim = 1; break;
        case 'x': o.exclude = optarg; break;
        case 'b': o.p.seg_rate = atoi(optarg); break;
        case 'I': o.include = optarg; break;
        case 'a': o.discarded_out = optarg; break;
        case 'A': o.discarded_in = optarg; break;
        case 'L': break;
        case 'w': o.p.multi = 1; break;
        case 'z': o.p.lowcov = atoi(optarg); break;
        case 'Y': o.p.merge_tips = atoi(optarg); break;
        case 'R':
          { const int flag = atoi(optarg);
            if (flag < 0 || flag > 6)
              { fprintf(stderr, "[ERROR]: Unsupported -R [%d] option.\n", flag);
                usage();
                exit(1);
              }
            o.p.remove |= 1 << flag;
            break;
          }
        case 'S': o.p.stitch_aggr = 1;       /* fall through */
        case 's': o.p.stitch = atoi(optarg); break;
        case 'v': o.verbose = 1; break;
        case 'p': o.purge = 1; break;
        case 'd': o.p.max_diffs = atof(optarg) / 100.0; break;
        case 'o': o.p.min_olen = atoi(optarg); break;
        case 'l': o.p.min_rlen = atoi(optarg); break;
        case 'u': o.p.max_unaligned = atoi(optarg); break;
        case 'n': o.p.min_nonrep = atoi(optarg); break;
        case 'r': o.rep_track = optarg; break;
        case 't': o.trim_track = optarg; break;
        case 'm': if (!unsupported) unsupported = "-m (repeat modules)"; break;
        case 'M': if (!unsupported) unsupported = "-M (repeat modules)"; break;
        case 'y': if (!unsupported) unsupported = "-y (repeat modules)"; break;
        case 'P': if (!unsupported) unsupported = "-P (repeat spanners)"; break;
        case 'Z': if (!unsupported) unsupported = "-Z (worst alignments)"; break;
        case 'D': if (!unsupported) unsupported = "-D (repeat interval analysis)"; break;
        case 'V': if (!unsupported) unsupported = "-V (repeat interval analysis)"; break;
        case 'W': if (!unsupported) unsupported = "-W (repeat interval analysis)"; break;
        case 'c': if (!unsupported) unsupported = "-c (chimer detection)"; break;
        case 'j': if (!unsupported) unsupported = "-j (obsolete indel trimming)"; break;
        default:
          fprintf(stderr, "[ERROR] unknown option -%c\n", optopt);
          usage();
          exit(1);
      }
  if (unsupported != NULL)
    { fprintf(stderr, "LAfilter: %s is not supported\n", unsupported);
      exit(1);
    }
  if (argc - optind != 3)
    { usage();
      exit(1);
    }
  rc = damar_filter_las(argv[optind], argv[optind + 1], argv[optind + 2], &o, &st);
  damar_filter_release();
  damar_box_release();
  return rc ? 1 : 0;
}
