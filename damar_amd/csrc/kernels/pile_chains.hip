/* pile_chains.hip -- LAseparate's per-group work for gfx950: the repeat counts of every record, the chains of every group
 * and the verdict on the best chain (scrub/LAseparate.c:146-193 getRepeatBases, :290-1081 chain, :1083-1372
 * separate_handler; the method itself is kernels/chain_core.h, which host/separate.c compiles too).
 *
 * Two kernels, one wavefront per pile, one wavefront per workgroup:
 *   record_marks   a lane per record.  Its two repeat counts, a loop over the few intervals of its reads; they depend on
 *                  nothing the chaining changes, so they are made once and not per extension step as in the reference.
 *                  The record of a group of one is judged here, which settles the great majority of the groups of a
 *                  daligner file.  The other records get the marks of a group's inner records (-1) and an empty member
 *                  list, which the second kernel overwrites where it has something to say.
 *   pile_chains    a lane per group of two or more records: the lane whose record begins the group walks it alone, since
 *                  the choice inside an extension step depends on the order the records are met in.  The three working
 *                  flags of the group's records are three 64-bit masks in the lane's registers; the chain being built, the
 *                  best chain so far (64 bytes each) and the ends and length keys of the earlier chains lie in the lane's
 *                  own slot of the workgroup's LDS.  The slots are an odd number of words apart, so that lanes at the same
 *                  place of their slots meet different banks.
 * The counts pass from the first kernel to the second through global memory, which the end of a kernel makes visible.
 * A wavefront's time is its worst lane's.  Groups are not dealt to wavefronts by size: that is unmeasured.
 * A group of more than maxgroup records, or one that finds more than maxchains valid chains or a chain of more than 64
 * members, is left to the host: status 1 at its first record, its other outputs are not to be looked at. */
#include "dev_common.h"
#include "damar_hip.h"
#include "kernels.h"

#define PC_THREADS    64
#define PC_MAX_BLOCKS 65536u
#define PC_SLOT_WORDS 113                 /* 64 + 64 bytes of members, DAMAR_SEPARATE_MAXCHAINS * 5 ints, one word to make it odd */

#define F_COMP    0x1                     /* lib/oflags.h */
#define F_DISCARD 0x2
#define F_TEMP    0x800
#define F_CONT    0x8000

typedef struct { u64 temp, cont, disc; } lane_state;
#define CH_FN    static __device__ __forceinline__
#define CH_MT    u8
#define CH_STATE lane_state
#define CH_MASK(s, bits)   ((((bits) & 1) ? (s)->temp : 0ull) | (((bits) & 2) ? (s)->cont : 0ull) | (((bits) & 4) ? (s)->disc : 0ull))
#define CH_IS(s, i, bits)  ((int) ((CH_MASK(s, bits) >> (i)) & 1ull))
#define CH_SET(s, i, bits) do { const u64 m_ = 1ull << (i); if ((bits) & 1) (s)->temp |= m_; if ((bits) & 2) (s)->cont |= m_; if ((bits) & 4) (s)->disc |= m_; } while (0)
#define CH_CLR(s, i, bits) do { const u64 m_ = ~(1ull << (i)); if ((bits) & 1) (s)->temp &= m_; if ((bits) & 2) (s)->cont &= m_; if ((bits) & 4) (s)->disc &= m_; } while (0)
#include "chain_core.h"

static_assert(PC_SLOT_WORDS * 4 >= 128 + 4 * CH_TAB_INTS * DAMAR_SEPARATE_MAXCHAINS, "a lane's slot holds its two member lists and its table");
static_assert(DAMAR_SEPARATE_MAXGROUP == 64, "the working flags of a group are 64-bit masks");

__global__ __launch_bounds__(PC_THREADS)
void record_marks(ChainArgs a)
{ const int l = lane_id();
  for (u32 p = blockIdx.x; p < a.npiles; p += gridDim.x)
    { const long long lo = a.pile_off[p];
      const int n = (int) (a.pile_off[p + 1] - lo);
      const int aread = a.pile_aread[p], alen = a.read_len[aread];
      const int *br = a.bread + lo;
      for (int i = l; i < n; i += WAVE)
        { const long long g = lo + i;
          const int bread = br[i], fl = a.flags[g];
          const int ab = a.abpos[g], ae = a.aepos[g], bb = a.bbpos[g], be = a.bepos[g];
          const bool head = (i == 0 || br[i - 1] != bread), alone = head && (i + 1 == n || br[i + 1] != bread);
          int ra = 0, rb = 0;
          if (a.rep_anno != NULL)
            ch_record_repeats(a.rep_anno, a.rep_data, aread, bread, ab, ae, bb, be, fl & F_COMP, &ra, &rb);
          a.arep[g] = ra;
          a.brep[g] = rb;
          a.o_best[g] = -1;
          a.status[g] = 0;
          if (alone)
            { const int proper = ch_single_proper(ab, ae, bb, be, alen, a.read_len[bread], a.kind);
              a.o_flags[g] = ((a.kind == 0 ? proper : !proper) ? (fl | F_DISCARD) : fl) & ~F_TEMP;
              a.o_nchains[g] = 0;
              a.o_proper[g] = proper;
              a.o_nbest[g] = 0;
            }
          else if (!head)
            a.o_nchains[g] = a.o_proper[g] = a.o_nbest[g] = -1;
        }
    }
}

__global__ __launch_bounds__(PC_THREADS)
void pile_chains(ChainArgs a)
{ __shared__ u32 s_slots[PC_THREADS * PC_SLOT_WORDS];
  const int l = lane_id();
  u8 *slot = (u8 *) (s_slots + l * PC_SLOT_WORDS);
  for (u32 p = blockIdx.x; p < a.npiles; p += gridDim.x)
    { const long long lo = a.pile_off[p];
      const int n = (int) (a.pile_off[p + 1] - lo);
      const int alen = a.read_len[a.pile_aread[p]];
      const int *br = a.bread + lo;
      for (int base = 0; base < n; base += WAVE)
        { const int i0 = base + l;
          if (i0 + 1 >= n || (i0 > 0 && br[i0] == br[i0 - 1]) || br[i0 + 1] != br[i0])
            continue;                         /* not the first record of a group of two or more */
          const int bread = br[i0];
          int g1 = i0 + 2;
          while (g1 < n && br[g1] == bread) g1++;
          const int gn = g1 - i0;
          const long long g = lo + i0;
          if (gn > a.maxgroup || gn > DAMAR_SEPARATE_MAXGROUP)
            { a.status[g] = 1;
              continue;
            }
          ch_recs r;
          r.ab = a.abpos + g;  r.ae = a.aepos + g;  r.bb = a.bbpos + g;  r.be = a.bepos + g;  r.fl = a.flags + g;
          r.arep = a.arep + g;  r.brep = a.brep + g;
          ch_work w;
          w.cur = slot;  w.best = slot + 64;  w.tab = (int *) (slot + 128);
          w.mcap = 64;
          w.maxchains = a.maxchains < DAMAR_SEPARATE_MAXCHAINS ? a.maxchains : DAMAR_SEPARATE_MAXCHAINS;
          lane_state s = { 0ull, 0ull, 0ull };
          for (int i = 0; i < gn; i++)
            { const int fi = r.fl[i];
              if (fi & F_CONT)    s.cont |= 1ull << i;
              if (fi & F_DISCARD) s.disc |= 1ull << i;
            }
          const int blen = a.read_len[bread];
          if (ch_chain(&r, gn, alen, blen, a.twidth, &s, &w))
            { a.status[g] = 1;
              continue;
            }
          a.o_proper[g] = ch_verdict(&r, gn, alen, blen, a.kind, &s, &w);
          a.o_nchains[g] = w.nchains;
          a.o_nbest[g] = w.nbest;
          for (int i = 0; i < gn; i++)
            { a.o_flags[g + i] = (r.fl[i] & ~(F_TEMP | F_CONT | F_DISCARD)) | (((s.temp >> i) & 1) ? F_TEMP : 0) | (((s.cont >> i) & 1) ? F_CONT : 0) |
                                 (((s.disc >> i) & 1) ? F_DISCARD : 0);
              if (i < w.nbest)
                a.o_best[g + i] = (int) w.best[i];
            }
        }
    }
}

void damar_launch_pile_chains(const ChainArgs *a, u32 grid, hipStream_t st)
{ if (a->npiles == 0)
    return;
  if (grid < 1 || grid > PC_MAX_BLOCKS)
    grid = PC_MAX_BLOCKS;
  const u32 blocks = a->npiles < grid ? a->npiles : grid;
  hipLaunchKernelGGL(record_marks, dim3(blocks), dim3(PC_THREADS), 0, st, *a);
  hipLaunchKernelGGL(pile_chains, dim3(blocks), dim3(PC_THREADS), 0, st, *a);
}

u32 damar_pile_chains_grid(void) { return PC_MAX_BLOCKS; }
