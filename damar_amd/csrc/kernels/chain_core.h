/* chain_core.h -- the chains of one group of overlaps (scrub/LAseparate.c chain(), :290-1081) and the verdict on its best
 * chain (:1083-1372) as integer code that the kernel (kernels/pile_chains.hip) and the host routine (host/separate.c) both
 * compile, as tile_core.h is: the host routine is the second opinion of the kernel in its storage and its limits, not in
 * its text.  (tests/separate_model.py is the opinion that shares no text.)  The includer sets
 *   CH_FN      the function qualifiers,
 *   CH_MT      the type of a chain member (an index into the group: a byte in the kernel, an int on the host),
 *   CH_STATE   the type that holds the three working flags of the group's records, with
 *   CH_IS(s, i, bits)  CH_SET(s, i, bits)  CH_CLR(s, i, bits)   over CH_TEMP, CH_CONT, CH_DISC.
 *
 * A group is the n consecutive records of one (A read, B read) in file order.  Nothing here depends on n beyond the room
 * of the work record: a chain that needs more members than mcap, or a group with more valid chains than maxchains, ends
 * with CH_ROOM and nothing of the result is valid.
 *
 * The reference is followed statement by statement where its output depends on the order of its statements: the choice
 * among the candidates of an extension step, the count of remaining records (which it lowers once per chain member a
 * bystander meets, so that it can end the search early), and the chain order (sorted only where the reference sorts). */
#ifndef DAMAR_CHAIN_CORE_H
#define DAMAR_CHAIN_CORE_H

#define CH_TEMP 1
#define CH_CONT 2
#define CH_DISC 4
#define CH_ANY  7
#define CH_ROOM 1

#define CH_LOOK_MIN    5000               /* LAseparate.c:293-295 */
#define CH_LOOK_MAX    30000
#define CH_LOOK_STRIDE 5000
#define CH_FILL_SLACK  100
#define CH_PROPER      1000
#define CH_TAB_INTS    5

typedef struct
{ const int *ab, *ae, *bb, *be, *fl;      /* the group's records; fl: the flags as they came (OVL_COMP is looked at) */
  const int *arep, *brep;                 /* getRepeatBases of the record for its A and its B read */
} ch_recs;

typedef struct
{ CH_MT *cur, *best;                      /* [mcap]: the chain being built, the first of the longest so far */
  int   *tab;                             /* [CH_TAB_INTS * maxchains]: first abpos, last aepos, first bbpos, last bepos, length key */
  int    mcap, maxchains;
  int    ncur, nbest, nchains, bestkey;
} ch_work;

CH_FN int ch_max(int a, int b) { return a > b ? a : b; }
CH_FN int ch_min(int a, int b) { return a < b ? a : b; }

CH_FN int ch_isect(int ab, int ae, int bb, int be)      /* lib/utils.c:250 */
{ const int b = ch_max(ab, bb), e = ch_min(ae, be);
  return b < e ? e - b : 0;
}

CH_FN int ch_within(int ab, int ae, int bb, int be) { return ab >= bb && ae <= be; }

/* getRepeatBases (:146-193) of the interval [b, e) over the intervals of one read */
CH_FN int ch_repeat_bases(const unsigned long long *anno, const int *data, int read, int b, int e)
{ unsigned long long t = anno[read] / sizeof(int);
  const unsigned long long te = anno[read + 1] / sizeof(int);
  int n = 0;
  for (; t < te; t += 2)
    n += ch_isect(b, e, data[t], data[t + 1]);
  return n;
}

/* the two counts of a record.  As the reference has it: a complemented B interval is mapped through the overlap's span
   (bepos - bbpos), not the read's length, and a self overlap takes A's coordinates for both reads. */
CH_FN void ch_record_repeats(const unsigned long long *anno, const int *data, int aread, int bread, int ab, int ae, int bb, int be, int comp,
                             int *arep, int *brep)
{ const int span = be - bb;
  *arep = ch_repeat_bases(anno, data, aread, ab, ae);
  if (aread == bread)
    *brep = *arep;
  else if (comp)
    *brep = ch_repeat_bases(anno, data, bread, span - be, span - bb);
  else
    *brep = ch_repeat_bases(anno, data, bread, bb, be);
}

/* a group of one record, and a group that chain() left without a chain: the first record alone is judged (:1198-1215, :1343-1363) */
CH_FN int ch_single_proper(int ab, int ae, int bb, int be, int alen, int blen, int kind)
{ const int pbeg = ch_min(ab, bb) < CH_PROPER, pend = (ae + CH_PROPER > alen || be + CH_PROPER > blen);
  if (kind == 0)
    return pbeg && pend;
  return (pbeg && pend) && !(ch_min(ab, bb) == 0 && (ae == alen || be == blen));
}

CH_FN int ch_push(ch_work *w, int i)
{ if (w->ncur >= w->mcap)
    return CH_ROOM;
  w->cur[w->ncur++] = (CH_MT) i;
  return 0;
}

/* cmp_ovls_abeg (:108-121) through a stable sort, as glibc's qsort is at these sizes */
CH_FN void ch_sort(const ch_recs *r, ch_work *w)
{ int i, j;
  for (i = 1; i < w->ncur; i++)
    { const int m = (int) w->cur[i], mb = r->ab[m], ml = r->ae[m] - r->ab[m];
      for (j = i; j > 0; j--)
        { const int q = (int) w->cur[j - 1];
          const int c = r->ab[q] != mb ? (r->ab[q] > mb) : (r->ae[q] - r->ab[q] > ml);
          if (!c)
            break;
          w->cur[j] = w->cur[j - 1];
        }
      w->cur[j] = (CH_MT) m;
    }
}

/* the seed extended to one side (:462-670 right, dir 1; :672-892 left, dir -1), a record at a time */
CH_FN int ch_extend(const ch_recs *r, int n, int top, int seed, int dir, CH_STATE *s, ch_work *w, int *nremain)
{ int ab1 = r->ab[seed], ae1 = r->ae[seed], bb1 = r->bb[seed], be1 = r->be[seed];
  int uoff = 1, ubases = -1, bases = -1, off = 1, its = top, i, step;
  for (;;)
    { for (step = CH_LOOK_MIN; step <= CH_LOOK_MAX && ubases == -1; step += CH_LOOK_STRIDE)
        for (i = seed + dir * uoff; i >= 0 && i < n; i += dir)
          { const int ab2 = r->ab[i], ae2 = r->ae[i], bb2 = r->bb[i], be2 = r->be[i];
            int ua, ub, x;
            if (((r->fl[i] ^ r->fl[seed]) & 1) || CH_IS(s, i, CH_ANY))
              continue;
            if (ch_within(ab2, ae2, ab1, ae1) || ch_within(bb2, be2, bb1, be1))
              continue;
            if (dir > 0)
              { if (ae2 < ae1 || be2 < be1)
                  continue;
                if (ch_max(ab2 - ae1, bb2 - be1) > step)
                  continue;
                if (ae1 - ab2 > ae2 - ae1 || be1 - bb2 > be2 - be1)       /* at least half of it overhangs */
                  continue;
              }
            else
              { if (ab2 > ab1 || bb2 > bb1)
                  continue;
                if (ch_max(ab1 - ae2, bb1 - be2) > step)
                  continue;
                if (ae2 - ab1 > ab1 - ab2 || be2 - bb1 > bb1 - bb2)
                  continue;
              }
            ua = (ae2 - ab2) - r->arep[i];
            ub = (be2 - bb2) - r->brep[i];
            x = ch_max(ch_isect(ab1, ae1, ab2, ae2), ch_isect(bb1, be1, bb2, be2));
            if (its > x && bases < ch_min(ae2 - ab2, be2 - bb2))
              { bases = ch_min(ae2 - ab2, be2 - bb2);
                off = dir * (i - seed);
                its = x;
              }
            if (ubases < ch_min(ua, ub))
              { uoff = dir * (i - seed);
                ubases = dir > 0 ? ch_min(ua, ub) : ua + ub;              /* the left side keeps the sum */
              }
            else if (ubases == -1 && step + CH_LOOK_STRIDE > CH_LOOK_MAX)  /* "for repetitive genomes": the best so far, as it stands now */
              { const int t = seed + dir * off;
                if (ch_isect(ab1, ae1, r->ab[t], r->ae[t]) < ae1 - r->ab[t] && ch_isect(bb1, be1, r->bb[t], r->be[t]) < be1 - r->bb[t])
                  { uoff = off;
                    ubases = 1;
                  }
              }
          }
      if (ubases < 0)
        return 0;
      i = seed + dir * uoff;
      if (ch_push(w, i))
        return CH_ROOM;
      CH_SET(s, i, CH_TEMP);
      *nremain -= 1;
      ab1 = r->ab[i];  ae1 = r->ae[i];  bb1 = r->bb[i];  be1 = r->be[i];
      uoff += 1;
      off = uoff;
      ubases = bases = -1;
      its = top;
      i = seed + dir * uoff;
      if (i < 0 || i >= n)
        return 0;
    }
}

/* cmp_chain_len's length (:78-106): the A spans, less one (the value of the comparison, not the intersection) per
   neighbouring pair that intersects */
CH_FN int ch_length_key(const ch_recs *r, const ch_work *w)
{ int len = 0, i;
  for (i = 0; i < w->ncur; i++)
    { const int m = (int) w->cur[i];
      len += r->ae[m] - r->ab[m];
      if (i > 0 && r->ae[(int) w->cur[i - 1]] > r->ab[m])
        len -= 1;
    }
  return len;
}

/* chain(): the state of the records comes in as OVL_CONT and OVL_DISCARD of the input (OVL_TEMP of the input is not looked
   at: no file holds it, and the reference's seed search would index before its array with it).  Leaves the state as the
   reference leaves the flags, w->nchains, and in w->best[0 .. nbest) the chain its sort puts first.  0 or CH_ROOM. */
CH_FN int ch_chain(const ch_recs *r, int n, int alen, int blen, int twidth, CH_STATE *s, ch_work *w)
{ const int top = ch_max(alen, blen);
  int nremain = n, i, j;
  w->ncur = w->nbest = w->nchains = 0;
  w->bestkey = 0;
  if (n < 2)
    return 0;
  for (i = 0; i < n; i++)
    { if (CH_IS(s, i, CH_CONT))
        continue;
      for (j = i + 1; j < n; j++)
        if (!CH_IS(s, j, CH_CONT) && ch_within(r->ab[j], r->ae[j], r->ab[i], r->ae[i]) && ch_within(r->bb[j], r->be[j], r->bb[i], r->be[i]))
          CH_SET(s, j, CH_CONT);
    }
  for (i = 0; i < n; i++)
    if (CH_IS(s, i, CH_CONT | CH_DISC))
      { CH_SET(s, i, CH_DISC);
        nremain -= 1;
      }
  while (nremain > 0)
    { int ubases = -1, useed = -1, lbases = -1, lseed = -1, seed, valid = 1, c;
      for (i = 0; i < n; i++)
        { int t;
          if (CH_IS(s, i, CH_ANY))
            continue;
          t = ch_max(r->ae[i] - r->ab[i] - r->arep[i], r->be[i] - r->bb[i] - r->brep[i]);
          if (t > ubases) { ubases = t;  useed = i; }
          t = ch_max(r->ae[i] - r->ab[i], r->be[i] - r->bb[i]);
          if (t > lbases) { lbases = t;  lseed = i; }
        }
      seed = (ubases < twidth && lbases > ubases) ? lseed : useed;
      if (seed < 0)                         /* not reached: nremain never exceeds the records that are left */
        break;
      w->ncur = 0;
      if (ch_push(w, seed))
        return CH_ROOM;
      CH_SET(s, seed, CH_TEMP);
      nremain -= 1;
      if (nremain && seed + 1 < n && ch_extend(r, n, top, seed, 1, s, w, &nremain))
        return CH_ROOM;
      if (nremain && seed > 0)
        { if (ch_extend(r, n, top, seed, -1, s, w, &nremain))
            return CH_ROOM;
          if (w->ncur > 1)
            ch_sort(r, w);
        }
      /* the records that fit a gap between two members (:905-961) */
      if (w->ncur > 1 && nremain > 0)
        { const int last = w->ncur - 1;
          int ci = 0;
          for (i = 0; i < n; i++)
            { if (CH_IS(s, i, CH_ANY) || ((r->fl[i] ^ r->fl[(int) w->cur[ci]]) & 1))
                continue;
              if (r->ab[i] < r->ab[(int) w->cur[ci]])
                continue;
              if (r->ab[i] > r->ab[(int) w->cur[last]])
                break;
              for (j = ci; j < last; j++)
                { const int p = (int) w->cur[j], q = (int) w->cur[j + 1];
                  if (r->ae[p] - CH_FILL_SLACK < r->ab[i] && r->ab[q] + CH_FILL_SLACK > r->ae[i] && r->be[p] - CH_FILL_SLACK < r->bb[i] &&
                      r->bb[q] + CH_FILL_SLACK > r->be[i])
                    { const int la = (int) w->cur[w->ncur - 1];
                      if (ch_isect(r->ab[i], r->ae[i], r->ab[la], r->ae[la]) > CH_FILL_SLACK ||
                          ch_isect(r->bb[i], r->be[i], r->bb[la], r->be[la]) > CH_FILL_SLACK)
                        break;
                      CH_SET(s, i, CH_TEMP);
                      if (ch_push(w, i))
                        return CH_ROOM;
                      nremain -= 1;
                    }
                  if (r->ab[i] > r->ab[q])
                    ci += 1;
                }
            }
          if (last < w->ncur - 1)
            ch_sort(r, w);
        }
      /* the bystanders that intersect a member (:963-993): the count goes down once per member met */
      if (nremain)
        { const int last = w->ncur - 1;
          int ci = 0;
          for (i = 0; i < n; i++)
            { if (CH_IS(s, i, CH_ANY) || ((r->fl[i] ^ r->fl[(int) w->cur[ci]]) & 1))
                continue;
              for (j = ci; j <= last; j++)
                { const int p = (int) w->cur[j];
                  if (ch_isect(r->ab[p], r->ae[p], r->ab[i], r->ae[i]) || ch_isect(r->bb[p], r->be[p], r->bb[i], r->be[i]))
                    { CH_SET(s, i, CH_DISC);
                      nremain -= 1;
                    }
                  if (j + 1 < w->ncur && r->ab[i] > r->ab[(int) w->cur[j + 1]])
                    ci += 1;
                }
            }
        }
      /* the sanity check (:998-1024).  The reference compares OVL_COMP of the new chain's first member with
         `flags && OVL_COMP` of the old one's, which is 1 for every member of a chain (it carries OVL_TEMP): a chain of
         complemented records is held against every earlier chain, another chain against none. */
      for (c = 0; c < w->nchains && valid; c++)
        { const int *t = w->tab + CH_TAB_INTS * c;
          if ((r->fl[(int) w->cur[0]] & 1) != 1)
            continue;
          for (j = 0; j < w->ncur; j++)
            { const int m = (int) w->cur[j];
              if ((r->ab[m] > t[0] && r->ae[m] < t[1]) || (r->bb[m] > t[2] && r->be[m] < t[3]))
                { valid = 0;
                  break;
                }
            }
        }
      if (valid)
        { const int first = (int) w->cur[0], last = (int) w->cur[w->ncur - 1], key = ch_length_key(r, w);
          int *t;
          if (w->nchains >= w->maxchains)
            return CH_ROOM;
          t = w->tab + CH_TAB_INTS * w->nchains;
          t[0] = r->ab[first];  t[1] = r->ae[last];  t[2] = r->bb[first];  t[3] = r->be[last];  t[4] = key;
          /* the sort at the end is stable and descending (:1065): its first chain is the first of the longest */
          if (w->nchains == 0 || key > w->bestkey)
            { for (j = 0; j < w->ncur; j++)
                w->best[j] = w->cur[j];
              w->nbest = w->ncur;
              w->bestkey = key;
            }
          w->nchains += 1;
        }
      else
        for (j = 0; j < w->ncur; j++)
          CH_SET(s, (int) w->cur[j], CH_DISC);
    }
  return 0;
}

/* whether the best chain is a proper one (:1094-1175 for kind 0, :1221-1313 for kind 1) */
CH_FN int ch_chain_proper(const ch_recs *r, const ch_work *w, int alen, int blen, int kind)
{ const int first = (int) w->best[0], last = (int) w->best[w->nbest - 1];
  int pbeg = ch_min(r->ab[first], r->bb[first]) < CH_PROPER;
  const int pend = (r->ae[last] + CH_PROPER > alen || r->be[last] + CH_PROPER > blen);
  int gap_a = 0, gap_b = 0, its_a = 0, its_b = 0, bases = 0, i;
  if (pbeg && pend)
    { if (kind == 1 && w->nbest == 1)
        { if (ch_min(r->ab[first], r->bb[first]) == 0 && (r->ae[first] == alen || r->be[first] == blen))
            pbeg = 0;
        }
      else
        { bases = ch_max(r->ae[first] - r->ab[first], r->be[first] - r->bb[first]);
          for (i = 1; i < w->nbest; i++)
            { const int p = (int) w->best[i - 1], m = (int) w->best[i];
              int xa = 0, xb = 0;
              bases += ch_max(r->ae[m] - r->ab[m], r->be[m] - r->bb[m]);
              if (r->ab[m] < r->ae[p])
                { xa = r->ae[p] - r->ab[m];
                  if (xa > CH_PROPER)
                    { its_a = -1;
                      break;
                    }
                  its_a += xa;
                }
              else
                gap_a += r->ab[m] - r->ae[p];
              if (r->bb[m] < r->be[p])
                { xb = r->be[p] - r->bb[m];
                  if (xb > CH_PROPER)
                    { its_b = -1;
                      break;
                    }
                  its_b += xb;
                }
              else
                gap_b += r->bb[m] - r->be[p];
              bases -= ch_max(xa, xb);
            }
        }
    }
  return pbeg && pend && its_a >= 0 && its_b >= 0 && gap_a >= 0 && gap_b >= 0 && bases * 0.3 > ch_max(gap_a, gap_b);
}

/* the verdict on a group after ch_chain (separate_handler, :1083-1372): the state's CH_DISC is what the first output file
   purges; returns whether the chain (without one: the first record) was found proper */
CH_FN int ch_verdict(const ch_recs *r, int n, int alen, int blen, int kind, CH_STATE *s, const ch_work *w)
{ int proper, i;
  if (w->nchains == 0)
    { proper = ch_single_proper(r->ab[0], r->ae[0], r->bb[0], r->be[0], alen, blen, kind);
      if (kind == 0 ? proper : !proper)
        CH_SET(s, 0, CH_DISC);
      return proper;
    }
  if (kind == 0)
    { proper = ch_chain_proper(r, w, alen, blen, 0);
      for (i = 0; i < n; i++)
        if (proper)
          CH_SET(s, i, CH_DISC);
        else
          CH_CLR(s, i, CH_DISC);
      return proper;
    }
  proper = (w->nchains == 1) && ch_chain_proper(r, w, alen, blen, 1);
  if (!proper)
    for (i = 0; i < n; i++)
      CH_SET(s, i, CH_DISC);
  return proper;
}

#endif
