! Capture wrapper for tests/golden/make_golden_ridge.py: bind(C) routines that set the module variables ridge_ice of the
! reference's ice_mechred reads, and call it on arrays handed in.  Compiled against the module files of the reference
! build (oracle/build_ref.sh, configuration small, or gx1 for --time) into a temporary library and linked to that
! build's library; nothing of it is committed but this text.
      module ridge_capture
      use iso_c_binding
      use ice_kinds_mod
      use ice_domain_size
      use ice_blocks, only: nx_block, ny_block
      implicit none
      contains

      subroutine rcap_set (ntr, dep, i_tsfc, i_alvl, i_vlvl, lvl, hmax, kpartic, kredist, mu, diag, ldiag) &
                 bind(C, name='rcap_set')
      use ice_state, only: ntrcr, trcr_depend, nt_Tsfc, nt_alvl, nt_vlvl
      use ice_itd, only: hin_max, ilyr1, slyr1
      use ice_mechred, only: krdg_partic, krdg_redist, mu_rdg, tr_lvl
      use ice_fileunits, only: nu_diag
      integer(c_int), value :: ntr, i_tsfc, i_alvl, i_vlvl, lvl, kpartic, kredist, ldiag
      real(c_double), value :: mu
      character(kind=c_char) :: diag(ldiag)   ! file that receives what the reference writes to nu_diag
      integer(c_int) :: dep(max_ntrcr)
      real(c_double) :: hmax(0:ncat)
      integer :: n
      character(len=1024) :: fname
      logical, save :: opened = .false.
      ntrcr = ntr
      trcr_depend(:) = dep(:)
      nt_Tsfc = i_tsfc
      nt_alvl = i_alvl
      nt_vlvl = i_vlvl
      tr_lvl = lvl /= 0
      krdg_partic = kpartic
      krdg_redist = kredist
      mu_rdg = mu
      hin_max(:) = hmax(:)                    ! (ridge_prep overwrites hin_max(ncat) with 1.0e8 at every call)
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
      end subroutine rcap_set

      ! with_opt = 0: the six optionals are absent
      subroutine rcap_ridge_ice (dt, icells, indxi, indxj, rdg_conv, rdg_shear, aicen, trcrn, vicen, vsnon, eicen, &
                 esnon, aice0, lstop, istop, jstop, dardg1dt, dardg2dt, dvirdgdt, opening, fresh, fhocn, with_opt) &
                 bind(C, name='rcap_ridge_ice')
      use ice_state, only: ntrcr, trcr_depend
      use ice_mechred, only: ridge_ice
      use ice_fileunits, only: nu_diag
      integer(c_int), value :: icells, with_opt
      real(c_double), value :: dt
      integer(c_int) :: indxi(nx_block*ny_block), indxj(nx_block*ny_block)
      integer(c_int) :: lstop, istop, jstop
      real(c_double) :: rdg_conv(nx_block,ny_block), rdg_shear(nx_block,ny_block), &
         aicen(nx_block,ny_block,ncat), trcrn(nx_block,ny_block,max_ntrcr,ncat), &
         vicen(nx_block,ny_block,ncat), vsnon(nx_block,ny_block,ncat), eicen(nx_block,ny_block,ntilyr), &
         esnon(nx_block,ny_block,ntslyr), aice0(nx_block,ny_block), dardg1dt(nx_block,ny_block), &
         dardg2dt(nx_block,ny_block), dvirdgdt(nx_block,ny_block), opening(nx_block,ny_block), &
         fresh(nx_block,ny_block), fhocn(nx_block,ny_block)
      logical (kind=log_kind) :: l_stop
      real (kind=dbl_kind), allocatable :: tr(:,:,:,:)
      allocate (tr(nx_block,ny_block,ntrcr,ncat))
      tr = trcrn(:,:,1:ntrcr,:)
      if (with_opt /= 0) then
         call ridge_ice (nx_block, ny_block, dt, ntrcr, icells, indxi, indxj, rdg_conv, rdg_shear, aicen, tr, &
                         vicen, vsnon, eicen, esnon, aice0, trcr_depend(1:ntrcr), l_stop, istop, jstop, &
                         dardg1dt, dardg2dt, dvirdgdt, opening, fresh, fhocn)
      else
         call ridge_ice (nx_block, ny_block, dt, ntrcr, icells, indxi, indxj, rdg_conv, rdg_shear, aicen, tr, &
                         vicen, vsnon, eicen, esnon, aice0, trcr_depend(1:ntrcr), l_stop, istop, jstop)
      endif
      trcrn(:,:,1:ntrcr,:) = tr
      lstop = merge(1, 0, l_stop)
      flush (nu_diag)
      end subroutine rcap_ridge_ice

      end module ridge_capture
