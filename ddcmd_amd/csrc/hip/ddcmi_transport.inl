/*
 * ddcmi_transport.inl -- everything that knows which transport a context has (compiled into ddcmi.hip, in front of
 * every other .inl).
 *
 * A decomposed run moves data between domains through the RCCL communicator (ctx->comm: production, and the loopback
 * bricks), through the host rendezvous (ctx->hcomm: TCP streams, the multi-process tests) or, inside an in-process group
 * (ctx->group_), by direct copies that ddcmi_multigpu.inl makes itself.  The fork between the first two lives here and
 * nowhere else: the predicates, the ranks' agreement on a rebuild's outcome, ONE point-to-point exchange over a message
 * table and the collectives.  ddcmi_preflight.inl is the one other file that calls RCCL and the rendezvous directly.
 */

/* ---- predicates -------------------------------------------------------------- */
static inline bool mg_transport(const ddcmi_ctx *ctx) { return ctx->comm != nullptr || ctx->hcomm != nullptr; }
/* this context's halo holds beads of other domains (loopback: a single rank whose periodic images count as such), whoever moves them */
static inline bool has_peers(const ddcmi_ctx *ctx) { return ctx->nranks > 1 || ctx->loopback; }
/* several domains, whoever moves the data */
static inline bool decomposed(const ddcmi_ctx *ctx) { return has_peers(ctx) || ctx->group_ != nullptr; }
/* this context exchanges through its transport (loopback: a single rank whose periodic images travel through it) */
static inline bool exchanging(const ddcmi_ctx *ctx) { return has_peers(ctx) && mg_transport(ctx); }
/* what ddcmi_comm_stats reports: 0 none, 1 RCCL, 2 host rendezvous, 3 RCCL loopback */
static inline int transport_kind(const ddcmi_ctx *ctx) { return ctx->comm ? (ctx->loopback ? 3 : 1) : ctx->hcomm ? 2 : 0; }

#define NCCLCHK2(ctx, call) do { ncclResult_t _r = (call); if (_r != ncclSuccess) SETERR(ctx, DDCMI_ECOMM, "%s failed: %s", #call, ncclGetErrorString(_r)); } while (0)
#define HOSTCHK(ctx, call) do { int _r = (call); if (_r != DDCMI_OK) SETERR(ctx, DDCMI_ECOMM, "%s failed: %s", #call, ddcmi_rdzv_last_error((ctx)->hcomm)); } while (0)

/* ---- leaving the job, and agreeing on a rebuild's outcome ------------------------ */
/* a rank that cannot go on at a point where its peers already wait for its data leaves the job: the host transport's
 * streams are closed (the peers' receives fail at once with "peer closed"), an RCCL communicator is aborted (peers inside
 * a kernel are released when the launcher tears the job down on this rank's non-zero exit) */
static int mg_fatal(ddcmi_ctx *ctx, int code, const char *msg)
{
   if (msg) ctx->err = msg;
   if (ctx->hcomm) ddcmi_rdzv_abort(ctx->hcomm);
   else if (ctx->comm) { (void)ncclCommAbort((ncclComm_t)ctx->comm); ctx->comm = nullptr; }
   return code;
}
/* the ranks agree on the outcome of a phase that has no count round behind it: max of the error codes (one small collective) */
static int mg_agree(ddcmi_ctx *ctx, int local_rc)
{
   if (!exchanging(ctx)) return local_rc;
   const std::string local_msg = ctx->err;
   hipStream_t st = ctx->stream;
   int worst = local_rc < 0 ? -local_rc : local_rc;
   if (ctx->hcomm)
   {
      double v = (double)worst;
      HOSTCHK(ctx, ddcmi_rdzv_allreduce_f64(ctx->hcomm, &v, 1, 1));
      worst = (int)v;
   }
   else
   {
      int *h = ctx->pinned(2, 64);
      if (!h) SETERR(ctx, DDCMI_ENOMEM, "pinned staging for the count exchange");
      ENSURE(ctx, ctx->cnt_xchg, 32);
      h[0] = worst;
      HIPCHK(ctx, hipMemcpyAsync(ctx->cnt_xchg.p, h, sizeof(int), hipMemcpyHostToDevice, st));
      NCCLCHK2(ctx, ncclAllReduce(ctx->cnt_xchg.p, ctx->cnt_xchg.p + 1, 1, ncclInt, ncclMax, (ncclComm_t)ctx->comm, st));
      PostJobs pj;
      pj.add(ctx->cnt_xchg.p + 1, 1);
      int rcp;
      if ((rcp = ddcmi_post(ctx, st, pj)) || (rcp = ddcmi_post_wait(ctx, st))) return rcp;
      worst = ctx->mbox.h[pj.off[0]];
   }
   if (local_rc) { ctx->err = local_msg; return local_rc; }
   if (worst) SETERR(ctx, DDCMI_ECOMM, "another rank failed during the list rebuild (error %d): its own message says why", worst);
   return DDCMI_OK;
}
/* The same agreement without anybody waiting for it (RCCL transport, rebuilds after the first two).  ADVICE r3: from the third
 * rebuild on a rank whose local phase failed (a bond stretched beyond the halo in a system going unstable, a capacity, an
 * allocation) used to abort its communicator and return, and its peers sat in the next halo kernel until something outside
 * killed the job.  Now every rank contributes its error code to an all-reduce (max) queued behind the phase's kernels, a post
 * kernel leaves the result in mapped host memory, and nobody waits: the failing rank returns its own error once the
 * collective has run; a healthy rank goes on queueing steps and looks at the word in front of its next host wait (ddcmi_agree_poll:
 * the next rebuild's count round, a read of energies, a download, ddcmi_sync) -- the word lands BEFORE the exchange the failed
 * peer never joins, so the look cannot hang, and a reported failure aborts the communicator (which releases the waiting
 * kernels) and returns DDCMI_ECOMM naming the rebuild.  Cost: one small collective per rebuild on the stream, no host wait. */
__global__ void k_agree_post(const int *src, int *dst, int seq)
{
   if (threadIdx.x == 0)
   {
      dst[1] = *src;
      __threadfence_system();
      __hip_atomic_store(dst, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
   }
}
static int mg_agree_async(ddcmi_ctx *ctx, int local_rc, int pretend_peer_code = 0 /* tests: the code a failed peer would have contributed */)
{
   hipStream_t st = ctx->stream;
   if (!ctx->agree.h)
   {
      if (ctx->agree.ensure(16, 0)) return mg_agree(ctx, local_rc);
      memset(ctx->agree.h, 0, 16 * sizeof(int));
   }
   { int rcp = ddcmi_agree_poll(ctx); if (rcp && !local_rc) return rcp; }      /* (never two agreements in flight) */
   const std::string local_msg = ctx->err;
   int *h = ctx->pinned(2, 64);
   if (!h) return mg_agree(ctx, local_rc);
   h[0] = std::max(local_rc < 0 ? -local_rc : local_rc, pretend_peer_code);
   int *d = ctx->d_flags + DDCMI_FLAG_AGREE;
   /* (a rebuild that went well contributes the zero its tail launch left there: no copy) */
   if (h[0] != 0 || !ctx->list_valid) HIPCHK(ctx, hipMemcpyAsync(d, h, sizeof(int), hipMemcpyHostToDevice, st));
   NCCLCHK2(ctx, ncclAllReduce(d, d + 1, 1, ncclInt, ncclMax, (ncclComm_t)ctx->comm, st));
   ctx->agree_seq++;
   hipLaunchKernelGGL(k_agree_post, dim3(1), dim3(64), 0, st, d + 1, ctx->agree.d, ctx->agree_seq);
   ctx->agree_pending = true; ctx->agree_loop = ctx->loop;
   if (local_rc)
   {
      /* this rank's own failure: it has told the others; it returns once the collective has run (its peers all join it) */
      (void)hipStreamSynchronize(st);
      ctx->agree_pending = false;
      ctx->err = local_msg;
      return local_rc;
   }
   return DDCMI_OK;
}
int ddcmi_agree_poll(ddcmi_ctx *ctx)
{
   if (!ctx->agree_pending) return DDCMI_OK;
   volatile int *flag = ctx->agree.h;
   struct timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
   for (unsigned long spin = 0;; spin++)
   {
      if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == ctx->agree_seq) break;
      if ((spin & 0xff) == 0xff)
      {
         struct timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
         if ((t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec) > 20.0)
         {
            ctx->agree_pending = false;
            return mg_fatal(ctx, DDCMI_ECOMM, "the ranks' agreement on the last list rebuild did not arrive within 20 s: a peer rank is gone");
         }
         sched_yield();
      }
   }
   ctx->agree_pending = false;
   const int worst = ctx->agree.h[1];
   if (worst)
   {
      char b[256];
      snprintf(b, sizeof(b), "another rank failed during the list rebuild at loop %lld (error %d): its own message says why", (long long)ctx->agree_loop, worst);
      return mg_fatal(ctx, DDCMI_ECOMM, b);      /* (aborting the communicator releases this rank's kernels that wait for the peer) */
   }
   return DDCMI_OK;
}

/* ---- point to point: one exchange over a message table ----------------------------- */
/* host transport: device segments -> host staging -> TCP streams -> host staging -> device segments */
static int mg_host_exchange(ddcmi_ctx *ctx, const HaloMsgs &ms, const double *sbase, const HaloMsgs &mr, double *rbase, int width, hipStream_t st)
{
   size_t stot = 0, rtot = 0;
   for (int k = 0; k < ms.n; k++) stot += (size_t)ms.cnt[k] * width;
   for (int k = 0; k < mr.n; k++) rtot += (size_t)mr.cnt[k] * width;
   ctx->hstage_s.resize(stot + 1); ctx->hstage_r.resize(rtot + 1);
   const void *sb[27]; void *rb[27]; size_t sbytes[27], rbytes[27];
   size_t o = 0;
   for (int k = 0; k < ms.n; k++)
   {
      double *s = ctx->hstage_s.data() + o;
      sb[k] = s; sbytes[k] = (size_t)ms.cnt[k] * width * sizeof(double); o += (size_t)ms.cnt[k] * width;
      HIPCHK(ctx, hipMemcpyAsync(s, sbase + (size_t)ms.off[k] * width, sbytes[k], hipMemcpyDeviceToHost, st));
   }
   HIPCHK(ctx, hipStreamSynchronize(st));
   o = 0;
   for (int k = 0; k < mr.n; k++) { rb[k] = ctx->hstage_r.data() + o; rbytes[k] = (size_t)mr.cnt[k] * width * sizeof(double); o += (size_t)mr.cnt[k] * width; }
   HOSTCHK(ctx, ddcmi_rdzv_exchange(ctx->hcomm, ms.n, ms.peer, sb, sbytes, mr.n, mr.peer, rb, rbytes));
   for (int k = 0; k < mr.n; k++) HIPCHK(ctx, hipMemcpyAsync(rbase + (size_t)mr.off[k] * width, rb[k], rbytes[k], hipMemcpyHostToDevice, st));
   HIPCHK(ctx, hipStreamSynchronize(st));      /* the staging vector is reused by the next exchange */
   return DDCMI_OK;
}
/* Message k of ms leaves sbase + ms.off[k] * width for rank ms.peer[k], message k of mr arrives at rbase + mr.off[k] * width from
 * rank mr.peer[k]; offsets and counts in items of `width` doubles, every count positive.  The sends are issued in table order and
 * so are the receives: in loopback a rank is its own peer, and RCCL pairs the k-th send to a peer with that peer's k-th receive
 * from it.  RCCL: one grouped launch on st, no host wait; host transport: staged through the host, with its waits. */
static int mg_exchange(ddcmi_ctx *ctx, const HaloMsgs &ms, const double *sbase, const HaloMsgs &mr, double *rbase, int width, hipStream_t st)
{
   if (ctx->hcomm) return mg_host_exchange(ctx, ms, sbase, mr, rbase, width, st);
   ncclComm_t comm = (ncclComm_t)ctx->comm;
   /* DDCMI_DEBUG_SPLIT_MSGS=<k> (with DDCMI_DEBUG_HOOKS=1, loopback only): every message travels as k send/recv pairs -- what a rank with k peers hands
    * RCCL per step (2x2x2: seven), on the one GPU there is to measure on: the same bytes, k times the operations of the group */
   static const int split_env = (getenv("DDCMI_DEBUG_HOOKS") && getenv("DDCMI_DEBUG_SPLIT_MSGS")) ? std::max(1, atoi(getenv("DDCMI_DEBUG_SPLIT_MSGS"))) : 1;
   const int split = ctx->loopback ? split_env : 1;
   NCCLCHK2(ctx, ncclGroupStart());
   for (int k = 0; k < ms.n; k++)
      for (int q = 0; q < split; q++)
      {
         const size_t a = (size_t)ms.cnt[k] * q / split, b = (size_t)ms.cnt[k] * (q + 1) / split;
         if (b > a) NCCLCHK2(ctx, ncclSend(sbase + ((size_t)ms.off[k] + a) * width, (b - a) * width, ncclDouble, ms.peer[k], comm, st));
      }
   for (int k = 0; k < mr.n; k++)
      for (int q = 0; q < split; q++)
      {
         const size_t a = (size_t)mr.cnt[k] * q / split, b = (size_t)mr.cnt[k] * (q + 1) / split;
         if (b > a) NCCLCHK2(ctx, ncclRecv(rbase + ((size_t)mr.off[k] + a) * width, (b - a) * width, ncclDouble, mr.peer[k], comm, st));
      }
   NCCLCHK2(ctx, ncclGroupEnd());
   return DDCMI_OK;
}

/* ---- collectives ------------------------------------------------------------- */
/* sum of n doubles on the device over the ranks, in place */
static int mg_allreduce_device(ddcmi_ctx *ctx, double *d, size_t n)
{
   if (n == 0 || !exchanging(ctx)) return DDCMI_OK;
   if (ctx->hcomm)
   {
      ctx->hstage_s.resize(n + 1);
      HIPCHK(ctx, hipMemcpyAsync(ctx->hstage_s.data(), d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      HOSTCHK(ctx, ddcmi_rdzv_allreduce_f64(ctx->hcomm, ctx->hstage_s.data(), (int)n, 0));
      HIPCHK(ctx, hipMemcpyAsync(d, ctx->hstage_s.data(), n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
      HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
      return DDCMI_OK;
   }
   NCCLCHK2(ctx, ncclAllReduce(d, d, n, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, ctx->stream));
   return DDCMI_OK;
}
/* sum of n doubles over the ranks, in place on the host */
static int mg_allreduce_host_values(ddcmi_ctx *ctx, double *values, int n)
{
   if (!exchanging(ctx)) return DDCMI_OK;
   if (ctx->hcomm) { HOSTCHK(ctx, ddcmi_rdzv_allreduce_f64(ctx->hcomm, values, n, 0)); return DDCMI_OK; }
   { int rca = ddcmi_agree_poll(ctx); if (rca) return rca; }
   double *d = ctx->d_results + R_GROUP;   /* scratch */
   HIPCHK(ctx, hipMemcpyAsync(d, values, n * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
   NCCLCHK2(ctx, ncclAllReduce(d, d, n, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, ctx->stream));
   HIPCHK(ctx, hipMemcpyAsync(values, d, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   return DDCMI_OK;
}
/* every rank's nv host doubles -> all[nranks * nv] on the host, in rank order; scratch: a device buffer of the caller's that the
 * RCCL side grows and passes through [sync] */
static int mg_allgather_host_values(ddcmi_ctx *ctx, const double *mine, double *all, size_t nv, dbuf<double> &scratch)
{
   if (ctx->hcomm) { HOSTCHK(ctx, ddcmi_rdzv_allgather(ctx->hcomm, mine, all, nv * sizeof(double))); return DDCMI_OK; }
   { int rca = ddcmi_agree_poll(ctx); if (rca) return rca; }
   ENSURE(ctx, scratch, ((size_t)ctx->nranks + 1) * nv);
   double *d = scratch.p;
   HIPCHK(ctx, hipMemcpyAsync(d, mine, nv * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
   NCCLCHK2(ctx, ncclAllGather(d, d + nv, nv, ncclDouble, (ncclComm_t)ctx->comm, ctx->stream));
   HIPCHK(ctx, hipMemcpyAsync(all, d + nv, (size_t)ctx->nranks * nv * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
   HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
   return DDCMI_OK;
}
/* The rebuild's count round (mg_counts_round): every rank's block of MG_BLK ints of the device counters dir_cnt -> all[MG_BLK * nranks]
 * on the host and, with_flags, this rank's d_flags -> h_flags; ONE host wait.  RCCL: the all-gather reads dir_cnt on the device, and
 * every rank's block (and this rank's flags) reach the host through the mailbox: no copy call that waits, no late wake-up (scan.hip).
 * Host transport: the block is downloaded into `stage` (MG_BLK pinned ints), then the rendezvous' all-gather. */
#define MG_BLK 32
static int mg_gather_counts(ddcmi_ctx *ctx, int *stage, int *all, bool with_flags)
{
   hipStream_t st = ctx->stream;
   const int nr = std::max(ctx->nranks, 1);
   if (ctx->hcomm)
   {
      if (with_flags) HIPCHK(ctx, hipMemcpyAsync(ctx->h_flags, ctx->d_flags, 8 * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(stage, ctx->dir_cnt.p, MG_BLK * sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HOSTCHK(ctx, ddcmi_rdzv_allgather(ctx->hcomm, stage, all, MG_BLK * sizeof(int)));
      return DDCMI_OK;
   }
   ENSURE(ctx, ctx->cnt_xchg, 32 + MG_BLK * (size_t)nr);
   NCCLCHK2(ctx, ncclAllGather(ctx->dir_cnt.p, ctx->cnt_xchg.p + 32, MG_BLK, ncclInt, (ncclComm_t)ctx->comm, st));
   PostJobs pj;
   pj.add(ctx->cnt_xchg.p + 32, MG_BLK * (size_t)nr).add(ctx->d_flags, 8);
   int rcp;
   if ((rcp = ddcmi_post(ctx, st, pj)) || (rcp = ddcmi_post_wait(ctx, st))) return rcp;
   memcpy(all, ctx->mbox.h + pj.off[0], MG_BLK * (size_t)nr * sizeof(int));
   if (with_flags) memcpy(ctx->h_flags, ctx->mbox.h + pj.off[1], 8 * sizeof(int));
   return DDCMI_OK;
}
