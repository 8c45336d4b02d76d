// The kernel template instances libsactd3_hip.so launches, as explicit instantiation definitions: this list, not the place where
// host code launches an instance, decides the order in which the compiler emits them -- and an instance's machine code has been
// seen to change with that order.  engine.hip includes the file once, behind all device code and in front of its first host function,
// so a host function may stand wherever it reads best.
//
// A new instance is APPENDED: every instance in front of it keeps its place.  One line per instance, spelled as c++filt prints the
// symbol (default template arguments written out, `T const*`).  tests/test_abi.py compares the list with the compiled code object:
// an instance that is launched but missing here is emitted behind the list and fails the test.  An instance listed here that
// nothing launches is still compiled and passes the test: that one is for the reviewer to catch.
template __global__ void k_nt<1, true, 2, 1, 2, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 2, 2, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 4, 2, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 1, 1, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 2, 1, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 4, 1, true>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 1, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 2, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 4, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 4, 1, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 1, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 4, 2, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 2, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 4, 4, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, true, 2, 4, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 1, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 2, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 4, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 4, 1, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 1, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 4, 2, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 2, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 4, 4, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, true, 2, 4, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, false, 2, 0, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, false, 2, 0, 2, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, false, 4, 0, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<1, false, 2, 0, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, false, 4, 0, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nt<2, false, 2, 0, 1, false>(int, int, int, int, int, int, int, int, DevCtl const*, NtArgs);
template __global__ void k_nn64<2, 2, 2>(NnArgs);
template __global__ void k_nn64<2, 2, 1>(NnArgs);
template __global__ void k_tn64<2, 2, 2, 1, 64>(Tn64Args);
template __global__ void k_adam_red_bc<true>(AdamRedArgs, BcFin);
template __global__ void k_adam_red_bc<false>(AdamRedArgs, BcFin);
template __global__ void k_adam_red<true>(AdamRedArgs);
template __global__ void k_adam_red<false>(AdamRedArgs);
template __global__ void k_tn_bc<2, true, true>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<1, true, true>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<2, false, true>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<1, false, true>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<2, true, false>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<1, true, false>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<2, false, false>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn_bc<1, false, false>(int, int, int, int, int, int, int, int, TnArgs, BcFin);
template __global__ void k_tn<2, true, true>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<1, true, true>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<2, false, true>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<1, false, true>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<2, true, false>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<1, true, false>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<2, false, false>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_tn<1, false, false>(int, int, int, int, int, int, int, int, TnArgs);
template __global__ void k_nt64<4, 2, 2>(NtArgs);
template __global__ void k_nt64_ln<4, 2, 2>(NtArgs);
template __global__ void k_nt64<2, 2, 1>(NtArgs);
template __global__ void k_nt64_ln<2, 2, 1>(NtArgs);
template __global__ void k_actor_tail_s<4>(ActorTail);
template __global__ void k_actor_tail_s2<4>(ActorTail, ActorTail, int);
template __global__ void k_ctail_nn<2>(CtailNn);
template __global__ void k_critic_tail<16>(CriticTail);
template __global__ void k_ln_bwd<16>(LnBwd);
template __global__ void k_qtail_nn<2>(QtailNn);
template __global__ void k_qtail_nn<1>(QtailNn);
template __global__ void k_actorq_tail<4>(ActorQTail);
template __global__ void k_actor_head_bwd_s<4>(ActorHeadBwd);
template __global__ void k_actor_head_bwd_s_bc<4>(ActorHeadBwd, BcArgs);
template __global__ void k_actor_tail_s5<4>(ActorTail5);
template __global__ void k_q_head<4>(QHead);
template __global__ void k_ctail_nn_w<2>(CtailNnW);
template __global__ void k_critic_tail_w<16>(CriticTailW);
template __global__ void k_mix_draw<false>(MixDrawArgs, MixCtl const*, int);
template __global__ void k_mix_draw<true>(MixDrawArgs, MixCtl const*, int);
