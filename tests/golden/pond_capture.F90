! Capture wrapper for tests/golden/make_golden_pond.py: bind(C) routines that set the module variables compute_ponds of the
! reference's ice_meltpond reads -- dt of ice_calendar, nt_Tsfc and nt_volpn of ice_state -- and call it and increment_age of
! ice_age on arrays handed in, one (block, category) at a time.  Compiled against the module files of the reference build
! (oracle/build_ref.sh, configuration small, or gx1 for --time) and of ice_meltpond, which the minter compiles from where
! it lies into its temporary directory; nothing of it is committed but this text.
      module pond_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine pdcap_set (dt_in, it_Tsfc, it_volpn) bind(C, name='pdcap_set')
      use ice_calendar, only: dt
      use ice_state, only: nt_Tsfc, nt_volpn
      real(c_double), value :: dt_in
      integer(c_int), value :: it_Tsfc, it_volpn
      dt = dt_in
      nt_Tsfc = it_Tsfc
      nt_volpn = it_volpn
      end subroutine pdcap_set

      subroutine pdcap_ponds (ilo, ihi, jlo, jhi, meltt, melts, frain, aicen, vicen, vsnon, trcrn, apondn, hpondn) &
                 bind(C, name='pdcap_ponds')
      use ice_meltpond, only: compute_ponds
      integer(c_int), value :: ilo, ihi, jlo, jhi
      real(c_double), dimension(nx_block,ny_block) :: meltt, melts, frain, aicen, vicen, vsnon, apondn, hpondn
      real(c_double) :: trcrn(nx_block,ny_block,max_ntrcr)
      call compute_ponds (nx_block, ny_block, ilo, ihi, jlo, jhi, meltt, melts, frain, aicen, vicen, vsnon, trcrn, &
                          apondn, hpondn)
      end subroutine pdcap_ponds

      subroutine pdcap_age (dt_in, icells, indxi, indxj, iage) bind(C, name='pdcap_age')
      use ice_age, only: increment_age
      real(c_double), value :: dt_in
      integer(c_int), value :: icells
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block)
      real(c_double) :: iage(nx_block,ny_block)
      call increment_age (nx_block, ny_block, dt_in, icells, indxi, indxj, iage)
      end subroutine pdcap_age

      end module pond_capture
