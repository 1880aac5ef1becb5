! Capture wrapper for tests/golden/make_golden_cleanup_itd.py: bind(C) routines that set the module variables cleanup_itd
! and aggregate of the reference's ice_itd read, and call them on arrays handed in.  Compiled against the module files
! of the reference build (oracle/build_ref.sh, configuration small, or gx1 for --time) into a temporary library and
! linked to that build's library; nothing of it is committed but this text.
      module cleanup_itd_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine ccap_set (ntr, dep, i_tsfc, hmax, diag, ldiag) bind(C, name='ccap_set')
      use ice_state, only: ntrcr, trcr_depend, nt_Tsfc
      use ice_itd, only: hin_max, ilyr1, slyr1
      use ice_fileunits, only: nu_diag
      integer(c_int), value :: ntr, i_tsfc, ldiag
      character(kind=c_char) :: diag(ldiag)   ! file that receives what the reference writes to nu_diag
      integer(c_int) :: dep(max_ntrcr)
      real(c_double) :: hmax(0:ncat)
      integer :: n
      character(len=1024) :: fname
      logical, save :: opened = .false.
      ntrcr = ntr
      trcr_depend(:) = dep(:)
      nt_Tsfc = i_tsfc
      hin_max(:) = hmax(:)
      do n = 1, ncat
         ilyr1(n) = (n-1)*nilyr + 1
         slyr1(n) = (n-1)*nslyr + 1
      enddo
      if (.not. opened) then
         nu_diag = 97
         fname = ' '
         do n = 1, min(ldiag, 1024)
            fname(n:n) = diag(n)
         enddo
         open (nu_diag, file=trim(fname), form='formatted')
         opened = .true.
      endif
      end subroutine ccap_set

      ! with_flux = 0: the three optional fluxes are absent
      subroutine ccap_cleanup_itd (ilo, ihi, jlo, jhi, dt, aicen, trcrn, vicen, vsnon, eicen, esnon, aice0, aice, &
                 fresh, fsalt, fhocn, with_flux, limit, lstop, istop, jstop) bind(C, name='ccap_cleanup_itd')
      use ice_state, only: ntrcr, trcr_depend
      use ice_itd, only: cleanup_itd
      use ice_fileunits, only: nu_diag
      integer(c_int), value :: ilo, ihi, jlo, jhi, with_flux, limit
      real(c_double), value :: dt
      integer(c_int) :: lstop, istop, jstop
      real(c_double) :: aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), &
         vicen(nx_block,ny_block,ncat), vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), &
         esnon(nx_block,ny_block,ntslyr), aice0(nx_block,ny_block), aice(nx_block,ny_block), &
         fresh(nx_block,ny_block), fsalt(nx_block,ny_block), fhocn(nx_block,ny_block)
      logical (kind=log_kind) :: l_stop
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      allocate (tr(nx_block,ny_block,ntrcr,ncat))
      tr = trcrn(:,:,1:ntrcr,:)
      if (with_flux /= 0) then
         call cleanup_itd (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, ntrcr, aicen, tr, vicen, vsnon, eicen, esnon, &
                           aice0, aice, trcr_depend(1:ntrcr), fresh, fsalt, fhocn, .true., l_stop, istop, jstop, &
                           limit_aice_in = (limit /= 0))
      else
         call cleanup_itd (nx_block, ny_block, ilo, ihi, jlo, jhi, dt, ntrcr, aicen, tr, vicen, vsnon, eicen, esnon, &
                           aice0, aice, trcr_depend(1:ntrcr), heat_capacity = .true., l_stop = l_stop, istop = istop, &
                           jstop = jstop, limit_aice_in = (limit /= 0))
      endif
      trcrn(:,:,1:ntrcr,:) = tr
      lstop = merge(1, 0, l_stop)
      flush (nu_diag)
      end subroutine ccap_cleanup_itd

      subroutine ccap_aggregate (aicen, trcrn, vicen, vsnon, eicen, esnon, aice, trcr, vice, vsno, eice, esno, aice0, &
                 tmask) bind(C, name='ccap_aggregate')
      use ice_state, only: ntrcr, trcr_depend
      use ice_itd, only: aggregate
      integer(c_int) :: tmask(nx_block,ny_block)
      real(c_double) :: aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), &
         vicen(nx_block,ny_block,ncat), vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), &
         esnon(nx_block,ny_block,ntslyr), aice(nx_block,ny_block), trcr(nx_block,ny_block,max_ntrcr), &
         vice(nx_block,ny_block), vsno(nx_block,ny_block), eice(nx_block,ny_block), esno(nx_block,ny_block), &
         aice0(nx_block,ny_block)
      logical (kind=log_kind) :: lmask(nx_block,ny_block)
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:), t1(:,:,:)
      lmask = tmask /= 0
      allocate (tr(nx_block,ny_block,ntrcr,ncat), t1(nx_block,ny_block,ntrcr))
      tr = trcrn(:,:,1:ntrcr,:)
      call aggregate (nx_block, ny_block, aicen, tr, vicen, vsnon, eicen, esnon, aice, t1, vice, vsno, eice, esno, &
                      aice0, lmask, ntrcr, trcr_depend(1:ntrcr))
      trcr(:,:,1:ntrcr) = t1
      end subroutine ccap_aggregate

      end module cleanup_itd_capture
